"""The reference's visibility test restated on the oracle's closest hit: what crt_intersect with CRT_INTERSECT_VISIBILITY must answer."""
import numpy as np


def _oracle_blocked(osc, o, d, lim):
    """blocked() of Render.cuh:19-27 from the oracle's closest hit (t = FLT_MAX on a miss)"""
    _, ot, _ = osc.intersect(o, d)
    with np.errstate(invalid="ignore", over="ignore"):
        return (lim.astype(np.float32) - ot) > np.float32(0.00001)
