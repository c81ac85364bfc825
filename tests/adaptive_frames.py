"""The fixed shape and settings of the adaptive-sampling GPU tests (tests/test_adaptive.py states what the restatement gives there), and
the GPU frame at them; tests/test_sample_map.py renders the same frame to feed its sample counts to crt_render_map."""
import cudaraytracing_amd as crt
import util

W, H, S = 37, 27, 29
AD = dict(min_samples=4, step_samples=6, threshold=0.2, mean_floor=0.01)


def gpu_adaptive(r, name, traversal=crt.TRAVERSAL_EXACT, want_variance=True, **kw):
    eye, iv, fov = util.camera(name)
    r.set_spp(S)
    r.seed, r.traversal = 0, traversal
    try:
        rgb = r.run_view_adaptive(eye, iv, fov, want_variance=want_variance, width=W, height=H, **dict(AD, **kw))
    finally:
        r.traversal = crt.TRAVERSAL_EXACT
    return dict(rgb=rgb, mean=r.mean_buffer, samples=r.samples_buffer, variance=r.variance_buffer, info=r.adaptive_info)
