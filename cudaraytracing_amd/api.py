"""Python mirror of the reference's Scene / Render / Task interface, a thin
layer over the C ABI (include/crt.h).  All work happens in libcrt.so: OBJ/MTL
ingestion and the BVH build in its C++ host layer, rendering in its HIP
kernels.  There is no Python or CPU rendering path.

reference: src/main.cu:40-90 (Task/config), include/Scene.h, include/Camera.h,
include/Render.cuh:357-557.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _capi as capi


def get_inverse_view_matrix(eye_pos, lookat, up):
    """reference: include/Camera.h:9-36.  Returns 9 floats, column-major."""
    e = np.asarray(eye_pos, dtype=np.float32)
    l = np.asarray(lookat, dtype=np.float32)
    u = np.asarray(up, dtype=np.float32)
    out = np.zeros(9, dtype=np.float32)
    capi.check(capi.lib().crt_inverse_view(capi.ptr(e), capi.ptr(l), capi.ptr(u), capi.ptr(out)), "crt_inverse_view")
    return out


def fov_to_radians(fov_y_deg):
    """reference: src/main.cu:278  `task.fov_y * (float)M_PI / 180` in float."""
    return np.float32(np.float32(np.float32(fov_y_deg) * np.float32(math.pi)) / np.float32(180))


class Task:
    """reference: struct Task + config_task(), src/main.cu:40-90."""

    def __init__(self, config_path, base_dir=None):
        t = capi.Task()
        capi.check(capi.lib().crt_task_load(os.fsencode(config_path), C.byref(t)), "crt_task_load")
        base = base_dir if base_dir is not None else os.getcwd()

        def res(p):
            p = p.decode()
            return p if os.path.isabs(p) else os.path.join(base, p)

        if t.n_objs <= 8:
            self.OBJ_paths = [(res(t.obj_path[i].value), res(t.mtl_dir[i].value)) for i in range(t.n_objs)]
        else:   # (any number of OBJ files, as src/main.cu:74-78 loops over them: the POD holds eight, crt_task_obj returns each)
            self.OBJ_paths = []
            for i in range(t.n_objs):
                o, m = C.create_string_buffer(4096), C.create_string_buffer(4096)
                capi.check(capi.lib().crt_task_obj(os.fsencode(config_path), i, o, m, 4096), "crt_task_obj")
                self.OBJ_paths.append((res(o.value), res(m.value)))
        self.lookat = np.array(t.lookat[:], dtype=np.float32)
        self.up = np.array(t.up[:], dtype=np.float32)
        self.eye_pos = np.array(t.eye_pos[:], dtype=np.float32)
        self.fov_y = np.float32(t.fov_y)
        self.width, self.height = int(t.width), int(t.height)
        self.bvh_thresh_n = int(t.bvh_thresh_n)
        self.light_sample_n = int(t.light_sample_n)
        self.P_RR = np.float32(t.p_rr)
        self.spp = int(t.spp)


class Scene:
    """reference: include/Scene.h:16-102 fed by Loader/Object (src/main.cu:122-145)."""

    def __init__(self, width, height):
        self._h = C.c_void_p()
        capi.check(capi.lib().crt_host_scene_create(width, height, C.byref(self._h)), "crt_host_scene_create")
        self.width, self.height = int(width), int(height)
        self._desc = None

    def add_obj(self, obj_path, mtl_dir):
        capi.check(capi.lib().crt_host_scene_add_obj(self._h, os.fsencode(obj_path), os.fsencode(mtl_dir)),
                   "crt_host_scene_add_obj")
        self._desc = None

    def set_BVH(self, thresh_n, device=None):
        """Scene::set_BVH (Scene.h:50-54).  device=None: the host builder; device=k: the same tree built on GPU k
        (byte-identical arrays, csrc/crt_bvh_build.hip), self.bvh_build_info says how it went."""
        if device is None:
            capi.check(capi.lib().crt_host_scene_set_bvh(self._h, thresh_n), "crt_host_scene_set_bvh")
            self.bvh_build_info = None
        else:
            info = capi.BvhBuildInfo()
            capi.check(capi.lib().crt_host_scene_set_bvh_device(self._h, thresh_n, device, C.byref(info)), "crt_host_scene_set_bvh_device")
            self.bvh_build_info = info.as_dict()
        self._desc = None

    def transform_object(self, index, m):
        """Moves object `index` (objects()' order) by the 3 x 4 affine map m (12 values, row-major), keeping the BVH's topology and
        refitting its boxes (crt_host_scene_transform_object); desc(), nodes(), triangles() ... then give the moved description, which
        Render.refit() pushes into a scene handle."""
        a = np.ascontiguousarray(m, dtype=np.float32).reshape(12)
        capi.check(capi.lib().crt_host_scene_transform_object(self._h, int(index), a.ctypes.data_as(C.POINTER(C.c_float))), "crt_host_scene_transform_object")
        self._desc = None

    def desc(self):
        if self._desc is None:
            d = capi.SceneDesc()
            capi.check(capi.lib().crt_host_scene_desc(self._h, C.byref(d)), "crt_host_scene_desc")
            self._desc = d
        return self._desc

    def _arr(self, p, n, dtype):
        if n == 0:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (n * dtype.itemsize)).from_address(C.addressof(p.contents))
        return np.frombuffer(buf, dtype=dtype).copy()

    def nodes(self):
        d = self.desc()
        return self._arr(d.nodes, d.n_nodes, capi.NODE_DTYPE)

    def triangles(self):
        d = self.desc()
        return self._arr(d.tris, d.n_tris, capi.TRI_DTYPE)

    def light_triangles(self):
        d = self.desc()
        return self._arr(d.light_tris, d.n_light_tris, capi.TRI_DTYPE)

    def materials(self):
        d = self.desc()
        return self._arr(d.materials, d.n_materials, capi.MAT_DTYPE)

    def lights(self):
        d = self.desc()
        return self._arr(d.lights, d.n_lights, capi.LIGHT_DTYPE)

    @property
    def root(self):
        return int(self.desc().root)

    def objects(self):
        n = C.c_uint32()
        capi.check(capi.lib().crt_host_scene_num_objects(self._h, C.byref(n)), "crt_host_scene_num_objects")
        out = []
        for i in range(n.value):
            a, l, c = C.c_float(), C.c_int32(), C.c_uint32()
            capi.check(capi.lib().crt_host_scene_object(self._h, i, C.byref(a), C.byref(l), C.byref(c)),
                       "crt_host_scene_object")
            out.append((bool(l.value), float(a.value), int(c.value)))
        return out

    def free(self):
        if self._h:
            capi.lib().crt_host_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    @classmethod
    def from_task(cls, task, width=None, height=None, bvh_device=None):
        """render_view()'s scene set-up (src/main.cu:119-145,276); bvh_device=k builds the BVH on GPU k (same arrays)."""
        s = cls(width or task.width, height or task.height)
        for obj, mtl in task.OBJ_paths:
            s.add_obj(obj, mtl)
        s.set_BVH(task.bvh_thresh_n, device=bvh_device)
        return s


class Render:
    """reference: class Render, include/Render.cuh:357-557.

    run_view renders on the GPU through crt_render (host buffers) or
    crt_render_device (device buffers, used by the multi-GPU path)."""

    def __init__(self, scene, spp=16, P_RR=0.8, light_sample_n=1, device=0):
        self.scene = scene
        self.spp, self.P_RR, self.light_sample_n = int(spp), np.float32(P_RR), int(light_sample_n)
        self.seed = 0
        self.traversal = capi.TRAVERSAL_EXACT
        self.extra_flags = 0  # e.g. FLAG_FORCE_EXACT (test hook)
        self.device = device
        self._h = C.c_void_p()
        capi.check(capi.lib().crt_scene_create(C.byref(scene.desc()), device, C.byref(self._h)), "crt_scene_create")
        self.frame_buffer = None
        self.mean_buffer = None
        self.stats = None
        self.aov_info = None
        self.aov_specular_info = None
        self.aov_direct_info = None
        self.aov_ao_info = None
        self.aov_buffers = None
        self.direct_buffers = None  # run_view_denoised with split_direct: direct and direct_variance of the frame
        self.shading_buffers = None  # run_view_denoised / run_view_temporal with demodulate: emission and diffuse_albedo of the frame
        self.denoise_info = None
        self.variance_buffer = None
        self.samples_buffer = None
        self.adaptive_info = None
        self.until_info = None
        self.refit_info = None
        self.map_info = None
        self.temporal_info = None
        self.variance_estimate_info = None
        self.low_frame = None            # run_view_upsampled: rgb, mean, variance, albedo, normal, depth (and the shading AOVs) of the low-resolution frame
        self.upsampled_variance = None
        self.upsample_info = None
        self.half_a_buffer = None        # run_view(want_halves=True): the means of the even and of the odd samples
        self.half_b_buffer = None
        self.filtered_rgb = None         # run_view(pixel_filter=True): the frame under the handle's pixel reconstruction filter
        self.filtered_mean = None
        self.select_buffers = None      # run_view_selected: choice, error, the halves, their variance and the filtered candidates
        self.select_info = None
        self.temporal_history_buffer = None
        self._temporal = None        # run_view_temporal: the history (temporal()'s `prev` dict), its camera and size
        self._temporal_frames = 0    # frames since the last reset_temporal()

    def _handle(self, what):
        """The crt_scene* of this renderer; raises when there is none (freed, or a MultiRender, whose handle is a crt_multi*)."""
        if not self._h:
            raise RuntimeError("%s: no single-device scene handle (freed, or a MultiRender)" % what)
        return self._h

    def accel_info(self):
        """How the acceleration trees of the FAST traversal were built (crt_scene_accel_info)."""
        self._handle("accel_info")
        a = capi.AccelInfo()
        capi.check(capi.lib().crt_scene_accel_info(self._h, C.byref(a)), "crt_scene_accel_info")
        return a.as_dict()

    # crt_scene_export's arrays (include/crt.h) and their element types: float4 rows as (n, 4) float32, int32 tables flat
    EXPORT_ARRAYS = {"nodes": np.float32, "nodes3": np.float32, "nodes4": np.float32, "nodes4i": np.float32, "leaf_geo": np.float32,
                     "leaf_geo_i": np.float32, "rec_map": np.int32, "tri_geo": np.float32, "leaf_count": np.int32, "tri_nm": np.float32}

    def export_trees(self):
        """Test hook: the traversal trees of this handle as the kernels read them, copied from device memory (crt_scene_export).
        Returns a dict of numpy arrays (float4 rows as (n, 4) float32, an absent array with 0 rows) and the crt_tree_scalars."""
        h = self._handle("export_trees")
        L = capi.lib()
        out = {}
        for name, dt in self.EXPORT_ARRAYS.items():
            n = C.c_size_t()
            capi.check(L.crt_scene_export(h, name.encode(), None, 0, C.byref(n)), "crt_scene_export")
            a = np.zeros(n.value // np.dtype(dt).itemsize, dtype=dt)
            if n.value:
                capi.check(L.crt_scene_export(h, name.encode(), capi.ptr(a), a.nbytes, C.byref(n)), "crt_scene_export")
            out[name] = a.reshape(-1, 4) if dt is np.float32 else a
        s = capi.TreeScalars()
        n = C.c_size_t()
        capi.check(L.crt_scene_export(h, b"scalars", C.byref(s), C.sizeof(s), C.byref(n)), "crt_scene_export")
        assert n.value == C.sizeof(s)
        out.update(s.as_dict())
        return out

    def export_array(self, name):
        """Test hook: one array of crt_scene_export by name -- those of EXPORT_ARRAYS, and "ltri" (the light triangles' rows) -- as
        export_trees() returns them."""
        h = self._handle("export_array")
        dt = self.EXPORT_ARRAYS.get(name, np.float32)
        n = C.c_size_t()
        capi.check(capi.lib().crt_scene_export(h, name.encode(), None, 0, C.byref(n)), "crt_scene_export")
        a = np.zeros(n.value // np.dtype(dt).itemsize, dtype=dt)
        if n.value:
            capi.check(capi.lib().crt_scene_export(h, name.encode(), capi.ptr(a), a.nbytes, C.byref(n)), "crt_scene_export")
        return a.reshape(-1, 4) if dt is np.float32 else a

    def refit(self, tris=None, light_tris=None):
        """Moves the handle's triangles without rebuilding it (crt_scene_refit): tris / light_tris are arrays of capi.TRI_DTYPE in the
        handle's BVH order / shape order, by default the scene's current ones (after Scene.transform_object).  Ends the frame in
        flight.  Returns crt_refit_info as a dict, also kept in self.refit_info."""
        h = self._handle("refit")
        t = np.ascontiguousarray(self.scene.triangles() if tris is None else tris, dtype=capi.TRI_DTYPE)
        l = np.ascontiguousarray(self.scene.light_triangles() if light_tris is None else light_tris, dtype=capi.TRI_DTYPE)
        info = capi.RefitInfo()
        capi.check(capi.lib().crt_scene_refit(h, capi.ptr(t), len(t), capi.ptr(l) if len(l) else None, len(l), C.byref(info)), "crt_scene_refit")
        self.refit_info = info.as_dict()
        return self.refit_info

    def refit_device(self, d_tris_ptr, d_light_tris_ptr, stream=None, n_tris=None, n_light_tris=None):
        """crt_scene_refit_device: the two arrays of crt_triangle (60 bytes each) are device pointers, e.g. tensor.data_ptr(); the work is
        enqueued on `stream` (a HIP stream handle as an integer; None: the null stream), which is synchronized once.  The counts default
        to the scene's."""
        h = self._handle("refit_device")
        nt = len(self.scene.triangles()) if n_tris is None else int(n_tris)
        nl = len(self.scene.light_triangles()) if n_light_tris is None else int(n_light_tris)
        info = capi.RefitInfo()
        capi.check(capi.lib().crt_scene_refit_device(h, C.c_void_p(d_tris_ptr), nt, C.c_void_p(d_light_tris_ptr) if d_light_tris_ptr else None, nl,
                                                     C.c_void_p(stream) if stream else None, C.byref(info)), "crt_scene_refit_device")
        self.refit_info = info.as_dict()
        return self.refit_info

    def set_spp(self, spp):
        self.spp = int(spp)

    def set_P_RR(self, p):
        self.P_RR = np.float32(p)

    def set_light_sample_n(self, n):
        self.light_sample_n = int(n)

    def _cam(self, eye_pos, inv_view_mat, fovY):
        return _camera(eye_pos, inv_view_mat, fovY)

    def _params(self, rank=0, world=1, flags=0, width=None, height=None):
        return capi.Params(width or self.scene.width, height or self.scene.height, self.spp, float(self.P_RR),
                           self.light_sample_n, self.seed, rank, world, self.traversal, flags)

    def _device_params(self, rank, world, tiled, width, height):
        """The crt_params of a device form: its shard, and the tiled output layout a shard of several always has"""
        return self._params(rank=rank, world=world, flags=(capi.FLAG_TILED_OUTPUT if (tiled or world > 1) else 0) | self.extra_flags,
                            width=width, height=height)

    def set_pixel_filter(self, spec):
        """The handle's pixel reconstruction filter (crt_set_pixel_filter, contract: include/crt.h): None for none, "box" (radius 0.5:
        the frame's own filter), "tent" (radius 1), "mitchell" (radius 2), or dict(kind=, radius=).  A setting the library does not
        allow raises CrtError and the handle keeps its old filter."""
        h_ = self._handle("set_pixel_filter")
        capi.check(capi.lib().crt_set_pixel_filter(h_, C.byref(_pixel_filter(spec)) if spec is not None else None), "crt_set_pixel_filter")

    def filtered(self, want_mean=True, width=None, height=None):
        """(rgb (H, W, 3), mean (H, W, 3) float32 or None, samples done) of crt_filtered_frame: the frame under the handle's pixel
        filter from the sums a render with pixel_filter=True keeps on the handle -- after the frame, or between the ranges of a
        progressive one.  Reads only."""
        h_ = self._handle("filtered")
        w, h = width or self.scene.width, height or self.scene.height
        rgb = np.zeros((h, w, 3), dtype=np.uint8)
        mean = np.zeros((h, w, 3), dtype=np.float32) if want_mean else None
        done = C.c_uint32(0)
        capi.check(capi.lib().crt_filtered_frame(h_, capi.ptr(rgb), capi.ptr(mean), C.byref(done)), "crt_filtered_frame")
        return rgb, mean, int(done.value)

    def run_view(self, eye_pos, inv_view_mat, fovY, stats=False, want_mean=True, width=None, height=None, want_variance=False, want_halves=False,
                 pixel_filter=False):
        """Renders the whole frame; returns the RGB8 frame buffer (H, W, 3).  want_variance: render with FLAG_VARIANCE (the frame is
        the same bits) and leave the per-pixel variance of the mean, (H, W, 3) float32 (crt_variance), in self.variance_buffer.
        want_halves: render with FLAG_HALF_BUFFERS (which implies FLAG_VARIANCE; the same bits again) and leave the means of the even
        and of the odd samples (crt_half_buffers) in self.half_a_buffer / self.half_b_buffer beside the variance.  pixel_filter: render
        with FLAG_PIXEL_FILTER (the same bits again; set_pixel_filter first) and leave the frame under the handle's filter
        (crt_filtered_frame) in self.filtered_rgb / self.filtered_mean."""
        if not self._h:
            raise RuntimeError("Render.run_view after free()")
        cam = self._cam(eye_pos, inv_view_mat, fovY)
        prm = self._params(flags=(capi.FLAG_STATS if stats else 0) | (capi.FLAG_VARIANCE if want_variance else 0) |
                           (capi.FLAG_HALF_BUFFERS if want_halves else 0) | (capi.FLAG_PIXEL_FILTER if pixel_filter else 0) | self.extra_flags,
                           width=width, height=height)
        w, h = prm.width, prm.height
        rgb = np.zeros((h, w, 3), dtype=np.uint8)
        mean = np.zeros((h, w, 3), dtype=np.float32) if want_mean else None
        st = capi.Stats()
        capi.check(capi.lib().crt_render(self._h, C.byref(cam), C.byref(prm), capi.ptr(rgb), capi.ptr(mean),
                                         C.byref(st)), "crt_render")
        self.frame_buffer, self.mean_buffer, self.stats = rgb, mean, st.as_dict()
        self.variance_buffer = self.variance(width=w, height=h)[0] if (want_variance or want_halves) else None
        self.half_a_buffer, self.half_b_buffer = self.half_buffers(width=w, height=h)[:2] if want_halves else (None, None)
        self.filtered_rgb, self.filtered_mean = self.filtered(width=w, height=h)[:2] if pixel_filter else (None, None)
        return rgb

    def half_buffers(self, width=None, height=None):
        """(a, b, samples done) of crt_half_buffers: the means of the even and of the odd samples of every pixel, (H, W, 3) float32 each,
        from the sums a render with want_halves keeps on the handle -- two independent estimates of the frame.  Reads only."""
        h_ = self._handle("half_buffers")
        w, h = width or self.scene.width, height or self.scene.height
        a, b = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w, 3), dtype=np.float32)
        done = C.c_uint32(0)
        capi.check(capi.lib().crt_half_buffers(h_, capi.ptr(a), capi.ptr(b), C.byref(done)), "crt_half_buffers")
        return a, b, int(done.value)

    def variance(self, width=None, height=None):
        """(var (H, W, 3) float32, samples done) of crt_variance: the estimated variance of the mean the frame -- or, between the ranges
        of a progressive render, the preview -- shows, from the sums a render with want_variance keeps on the handle.  Reads only."""
        h_ = self._handle("variance")
        w, h = width or self.scene.width, height or self.scene.height
        var = np.zeros((h, w, 3), dtype=np.float32)
        done = C.c_uint32(0)
        capi.check(capi.lib().crt_variance(h_, capi.ptr(var), C.byref(done)), "crt_variance")
        return var, int(done.value)

    def run_view_adaptive(self, eye_pos, inv_view_mat, fovY, min_samples=None, step_samples=None, threshold=None, mean_floor=None,
                          want_variance=False, width=None, height=None):
        """Variance-driven adaptive sampling (crt_render_adaptive, contract: include/crt.h): every pixel gets min_samples samples, then
        step_samples more per pass until the standard error of its mean is at most threshold x (mean + mean_floor) or it has all
        self.spp.  None settings take crt_adaptive_defaults.  Returns the RGB8 frame (H, W, 3); self.mean_buffer is its mean,
        self.samples_buffer the samples per pixel (H, W) uint32, self.variance_buffer (want_variance) the variance of that mean
        (H, W, 3), self.adaptive_info the crt_adaptive_info dict.  Ends a progressive render in flight on the handle."""
        h_ = self._handle("run_view_adaptive")
        cam = self._cam(eye_pos, inv_view_mat, fovY)
        prm = self._params(flags=self.extra_flags, width=width, height=height)
        ap = _adaptive_params(min_samples, step_samples, threshold, mean_floor)
        w, h = prm.width, prm.height
        rgb = np.zeros((h, w, 3), dtype=np.uint8)
        mean = np.zeros((h, w, 3), dtype=np.float32)
        samples = np.zeros((h, w), dtype=np.uint32)
        var = np.zeros((h, w, 3), dtype=np.float32) if want_variance else None
        info = capi.AdaptiveInfo()
        capi.check(capi.lib().crt_render_adaptive(h_, C.byref(cam), C.byref(prm), C.byref(ap), capi.ptr(rgb), capi.ptr(mean), capi.ptr(samples),
                                                  capi.ptr(var), C.byref(info)), "crt_render_adaptive")
        self.frame_buffer, self.mean_buffer, self.samples_buffer, self.variance_buffer = rgb, mean, samples, var
        self.adaptive_info = info.as_dict()
        return rgb

    def _map_frame(self, what, call, prm, want_variance):
        """The host form of a call that writes crt_render_map's outputs: call(rgb, mean, samples, var, info) -> status"""
        w, h = prm.width, prm.height
        rgb = np.zeros((h, w, 3), dtype=np.uint8)
        mean = np.zeros((h, w, 3), dtype=np.float32)
        samples = np.zeros((h, w), dtype=np.uint32)
        var = np.zeros((h, w, 3), dtype=np.float32) if want_variance else None
        info = capi.MapInfo()
        capi.check(call(capi.ptr(rgb), capi.ptr(mean), capi.ptr(samples), capi.ptr(var), C.byref(info)), what)
        self.frame_buffer, self.mean_buffer, self.samples_buffer, self.variance_buffer = rgb, mean, samples, var
        self.map_info = info.as_dict()
        return rgb

    def run_view_map(self, eye_pos, inv_view_mat, fovY, sample_map, sample_begin=0, want_variance=False, width=None, height=None):
        """A frame with a caller-given number of samples per pixel (crt_render_map, contract: include/crt.h): pixel p gets samples
        sample_begin .. n_p - 1 of self.spp, n_p = min(max(sample_map[p], max(sample_begin, 1)), spp); sample_map is (H, W), any integer
        type.  sample_begin > 0 continues the frame in flight (run_view_range(0, sample_begin, want_variance=True)).  Returns the RGB8
        frame (H, W, 3); self.mean_buffer is its mean, self.samples_buffer the samples per pixel (H, W) uint32, self.variance_buffer
        (want_variance) the variance of that mean, self.map_info the crt_map_info dict.  No frame is in flight afterwards."""
        h_ = self._handle("run_view_map")
        cam = self._cam(eye_pos, inv_view_mat, fovY)
        prm = self._params(flags=self.extra_flags, width=width, height=height)
        m = np.ascontiguousarray(sample_map, dtype=np.uint32)
        if m.shape != (prm.height, prm.width):
            raise ValueError("run_view_map needs an (H, W) = (%d, %d) sample map, got %r" % (prm.height, prm.width, m.shape))
        return self._map_frame("crt_render_map", lambda rgb, mean, samples, var, info: capi.lib().crt_render_map(
            h_, C.byref(cam), C.byref(prm), capi.ptr(m), int(sample_begin), rgb, mean, samples, var, info), prm, want_variance)

    def run_view_planned(self, eye_pos, inv_view_mat, fovY, min_samples=None, threshold=None, mean_floor=None, want_variance=False,
                         width=None, height=None):
        """The adaptive frame in two launches (crt_render_planned): min_samples samples of every pixel, the sample plan made from their
        variance (sample_plan), the rest of every pixel's samples in one launch per chunk.  None settings take crt_adaptive_defaults.
        Results as run_view_map; self.map_info counts the warm-up's paths and launches too."""
        h_ = self._handle("run_view_planned")
        cam = self._cam(eye_pos, inv_view_mat, fovY)
        prm = self._params(flags=self.extra_flags, width=width, height=height)
        ap = _adaptive_params(min_samples, None, threshold, mean_floor)
        return self._map_frame("crt_render_planned", lambda rgb, mean, samples, var, info: capi.lib().crt_render_planned(
            h_, C.byref(cam), C.byref(prm), C.byref(ap), rgb, mean, samples, var, info), prm, want_variance)

    def sample_plan(self, threshold=None, mean_floor=None, width=None, height=None):
        """(map (H, W) uint32, samples done) of crt_sample_plan: the samples each pixel needs for the standard error of its mean to
        reach threshold x (mean + mean_floor), from the sums of the frame in flight (ranges with want_variance).  Reads only; the map
        is what run_view_map takes with sample_begin = samples done.  None settings take crt_adaptive_defaults."""
        h_ = self._handle("sample_plan")
        ap = _adaptive_params(None, None, threshold, mean_floor)
        w, h = width or self.scene.width, height or self.scene.height
        m = np.zeros((h, w), dtype=np.uint32)
        info = capi.PlanInfo()
        capi.check(capi.lib().crt_sample_plan(h_, ap.threshold, ap.mean_floor, capi.ptr(m), C.byref(info)), "crt_sample_plan")
        return m, int(info.samples)

    def frame_error(self, threshold=None, mean_floor=None):
        """The error of the frame in flight (or of the last finished frame) as a FrameError (crt_frame_error, contract: include/crt.h):
        the sums a render with want_variance keeps on the handle, reduced on the device over the shard's pixels against the adaptive
        call's target, standard error <= threshold x (mean + mean_floor).  Reads only.  None settings take crt_frame_error_defaults."""
        h_ = self._handle("frame_error")
        thr, floor = _frame_error_settings(threshold, mean_floor)
        info = capi.FrameErrorInfo()
        capi.check(capi.lib().crt_frame_error(h_, thr, floor, C.byref(info)), "crt_frame_error")
        return FrameError(info.as_dict(), thr, floor)

    def frame_error_device(self, d_out_ptr, threshold=None, mean_floor=None, stream=None):
        """crt_frame_error_device: the crt_frame_error_info into the device buffer d_out_ptr (capi.FrameErrorInfo's layout), enqueued on
        `stream` without synchronizing."""
        h_ = self._handle("frame_error_device")
        thr, floor = _frame_error_settings(threshold, mean_floor)
        capi.check(capi.lib().crt_frame_error_device(h_, thr, floor, C.c_void_p(d_out_ptr), C.c_void_p(stream) if stream else None), "crt_frame_error_device")

    def _until_params(self, prm, min_samples, step_samples, threshold, mean_floor, max_above):
        """crt_until_params from the settings (None: crt_until_defaults'); max_above: a pixel count (int) or a fraction of the shard's
        pixels (float below 1)"""
        up = capi.UntilParams()
        capi.check(capi.lib().crt_until_defaults(C.byref(up)), "crt_until_defaults")
        for name, v in (("min_samples", min_samples), ("step_samples", step_samples), ("threshold", threshold), ("mean_floor", mean_floor)):
            if v is not None:
                setattr(up, name, int(v) if name.endswith("samples") else float(v))
        if max_above is not None:
            if isinstance(max_above, (float, np.floating)):
                if not 0.0 <= max_above < 1.0:
                    raise ValueError("run_view_until: a fractional max_above must be in [0, 1), got %r" % (max_above,))
                max_above = int(float(max_above) * shard_pixels(prm.width, prm.height, prm.rank, prm.world))
            up.max_above = int(max_above)
        return up

    def run_view_until(self, eye_pos, inv_view_mat, fovY, min_samples=None, step_samples=None, threshold=None, mean_floor=None, max_above=None,
                       sample_begin=0, want_variance=False, want_mean=True, want_halves=False, width=None, height=None):
        """A uniform frame rendered until it is clean enough (crt_render_until, contract: include/crt.h): min_samples samples of every
        pixel, then step_samples more per range until at most max_above pixels (an int, or a fraction of the pixels as a float) have a
        standard error above threshold x (mean + mean_floor), or all self.spp samples are in.  None settings take crt_until_defaults.
        Returns the RGB8 frame (H, W, 3): run_view's bits when the frame ran to spp, else preview()'s at the samples done -- and then
        the frame STAYS IN FLIGHT: run_view_range or run_view_until(sample_begin=samples done) continues it.  self.mean_buffer
        (want_mean) and self.variance_buffer (want_variance) go with it; self.until_info is the crt_until_info dict, its "last" a
        FrameError.  want_halves: the ranges go with FLAG_HALF_BUFFERS."""
        h_ = self._handle("run_view_until")
        cam = self._cam(eye_pos, inv_view_mat, fovY)
        prm = self._params(flags=(capi.FLAG_HALF_BUFFERS if want_halves else 0) | self.extra_flags, width=width, height=height)
        up = self._until_params(prm, min_samples, step_samples, threshold, mean_floor, max_above)
        w, h = prm.width, prm.height
        rgb = np.zeros((h, w, 3), dtype=np.uint8)
        mean = np.zeros((h, w, 3), dtype=np.float32) if want_mean else None
        var = np.zeros((h, w, 3), dtype=np.float32) if want_variance else None
        info = capi.UntilInfo()
        capi.check(capi.lib().crt_render_until(h_, C.byref(cam), C.byref(prm), C.byref(up), int(sample_begin), capi.ptr(rgb), capi.ptr(mean), capi.ptr(var),
                                               C.byref(info)), "crt_render_until")
        self.frame_buffer, self.mean_buffer, self.variance_buffer = rgb, mean, var
        self.until_info = _until_info(info, up)
        return rgb

    def run_view_until_device(self, eye_pos, inv_view_mat, fovY, ptrs, min_samples=None, step_samples=None, threshold=None, mean_floor=None,
                              max_above=None, sample_begin=0, stream=None, rank=0, world=1, tiled=False, want_info=True, width=None, height=None):
        """crt_render_until_device: ptrs = {"rgb", "mean", "variance": raw device pointer or None} (row-major, or the shard's compact
        tiles with tiled / world > 1), work enqueued on `stream`.  The call synchronizes the stream once per check (once more with
        want_info, which sets self.until_info)."""
        h_ = self._handle("run_view_until_device")
        cam = self._cam(eye_pos, inv_view_mat, fovY)
        prm = self._device_params(rank, world, tiled, width, height)
        up = self._until_params(prm, min_samples, step_samples, threshold, mean_floor, max_above)
        info = capi.UntilInfo()
        out = [C.c_void_p(ptrs[n]) if ptrs.get(n) else None for n in ("rgb", "mean", "variance")]
        capi.check(capi.lib().crt_render_until_device(h_, C.byref(cam), C.byref(prm), C.byref(up), int(sample_begin), *out,
                                                      C.c_void_p(stream) if stream else None, C.byref(info) if want_info else None), "crt_render_until_device")
        if want_info:
            self.until_info = _until_info(info, up)
        return self.until_info if want_info else None

    def _map_device(self, what, call, ptrs, stream, want_info):
        info = capi.MapInfo()
        out = [C.c_void_p(ptrs[n]) if ptrs.get(n) else None for n in ("rgb", "mean", "samples", "variance")]
        capi.check(call(*out, C.c_void_p(stream) if stream else None, C.byref(info) if want_info else None), what)
        if want_info:
            self.map_info = info.as_dict()
        return self.map_info if want_info else None

    def run_view_map_device(self, eye_pos, inv_view_mat, fovY, d_map_ptr, ptrs, sample_begin=0, stream=None, rank=0, world=1, tiled=False,
                            want_info=True, width=None, height=None):
        """crt_render_map_device: d_map_ptr a raw device pointer to the (H, W) uint32 map, ptrs = {"rgb", "mean", "samples", "variance":
        raw device pointer or None} (row-major, or the shard's compact tiles with tiled / world > 1), work enqueued on `stream`.  The
        call synchronizes the stream once (twice with want_info, which sets self.map_info)."""
        h_ = self._handle("run_view_map_device")
        cam = self._cam(eye_pos, inv_view_mat, fovY)
        prm = self._device_params(rank, world, tiled, width, height)
        return self._map_device("crt_render_map_device", lambda rgb, mean, samples, var, st, info: capi.lib().crt_render_map_device(
            h_, C.byref(cam), C.byref(prm), C.c_void_p(d_map_ptr), int(sample_begin), rgb, mean, samples, var, st, info), ptrs, stream, want_info)

    def run_view_planned_device(self, eye_pos, inv_view_mat, fovY, ptrs, min_samples=None, threshold=None, mean_floor=None, stream=None,
                                rank=0, world=1, tiled=False, want_info=True, width=None, height=None):
        """crt_render_planned_device: outputs and synchronization as run_view_map_device."""
        h_ = self._handle("run_view_planned_device")
        cam = self._cam(eye_pos, inv_view_mat, fovY)
        prm = self._device_params(rank, world, tiled, width, height)
        ap = _adaptive_params(min_samples, None, threshold, mean_floor)
        return self._map_device("crt_render_planned_device", lambda rgb, mean, samples, var, st, info: capi.lib().crt_render_planned_device(
            h_, C.byref(cam), C.byref(prm), C.byref(ap), rgb, mean, samples, var, st, info), ptrs, stream, want_info)

    def run_view_range(self, eye_pos, inv_view_mat, fovY, sample_begin, sample_count, want_mean=True, width=None, height=None,
                       want_variance=False, stats=False, want_halves=False, pixel_filter=False):
        """Progressive rendering: adds samples [sample_begin, sample_begin + sample_count) of the spp samples per pixel to the
        accumulator of the device scene; ranges go in ascending order from 0.  Returns the RGB8 frame once the range that ends
        at spp has been rendered (bit-identical to run_view), None before.  A range with sample_begin > 0 that does not continue
        the frame in flight on the handle (samples so far, spp, size) raises CrtError.  want_halves: the range goes with
        FLAG_HALF_BUFFERS (half_buffers() reads the halves between the ranges and after the last).  pixel_filter: the range goes
        with FLAG_PIXEL_FILTER (filtered() reads the filtered frame between the ranges and after the last)."""
        if not self._h:
            raise RuntimeError("Render.run_view_range after free()")
        cam = self._cam(eye_pos, inv_view_mat, fovY)
        prm = self._params(flags=(capi.FLAG_STATS if stats else 0) | (capi.FLAG_VARIANCE if want_variance else 0) |
                           (capi.FLAG_HALF_BUFFERS if want_halves else 0) | (capi.FLAG_PIXEL_FILTER if pixel_filter else 0) | self.extra_flags,
                           width=width, height=height)
        w, h = prm.width, prm.height
        last = sample_begin + sample_count == self.spp
        rgb = np.zeros((h, w, 3), dtype=np.uint8) if last else None
        mean = np.zeros((h, w, 3), dtype=np.float32) if (last and want_mean) else None
        st = capi.Stats()
        capi.check(capi.lib().crt_render_range(self._h, C.byref(cam), C.byref(prm), int(sample_begin), int(sample_count),
                                               capi.ptr(rgb) if last else None, capi.ptr(mean), C.byref(st)), "crt_render_range")
        self.stats = st.as_dict()
        if last:
            self.frame_buffer, self.mean_buffer = rgb, mean
        return rgb

    def last_launch_ms(self):
        """(device ms, launches) of the render kernel of the last frame submitted on this handle (crt_last_launch_ms); the frame's
        stream must have been synchronized."""
        ms, n = C.c_float(), C.c_uint32()
        capi.check(capi.lib().crt_last_launch_ms(self._handle("last_launch_ms"), C.byref(ms), C.byref(n)), "crt_last_launch_ms")
        return float(ms.value), int(n.value)

    def item_order(self):
        """{"lists_built", "lists_reused", "classes", "window"} of the handle (crt_item_order): how often a launch of the render kernel
        built the order of its last work items and how often it found it built; classes and window of the last launch."""
        info = capi.ItemOrderInfo()
        capi.check(capi.lib().crt_item_order(self._handle("item_order"), C.byref(info)), "crt_item_order")
        return {"lists_built": int(info.lists_built), "lists_reused": int(info.lists_reused), "classes": int(info.classes), "window": int(info.window)}

    def radiance_storage(self):
        """(bytes, ring samples) of the per-path radiance storage of the last render on this handle (crt_radiance_storage): one value per
        path of a chunk, or -- FLAG_BOUNDED_RADIANCE -- a ring of that many samples."""
        b, r = C.c_uint64(), C.c_uint32()
        capi.check(capi.lib().crt_radiance_storage(self._handle("radiance_storage"), C.byref(b), C.byref(r)), "crt_radiance_storage")
        return int(b.value), int(r.value)

    def preview(self, want_mean=False, width=None, height=None):
        """Displayable frame of the progressive render in flight (crt_preview): returns (rgb (H, W, 3), mean or None, samples done).
        Reads the accumulator only -- the final frame does not depend on previews."""
        if not self._h:
            raise RuntimeError("Render.preview after free()")
        w, h = width or self.scene.width, height or self.scene.height
        rgb = np.zeros((h, w, 3), dtype=np.uint8)
        mean = np.zeros((h, w, 3), dtype=np.float32) if want_mean else None
        done = C.c_uint32(0)
        capi.check(capi.lib().crt_preview(self._h, capi.ptr(rgb), capi.ptr(mean), C.byref(done)), "crt_preview")
        return rgb, mean, int(done.value)

    def run_view_device(self, eye_pos, inv_view_mat, fovY, d_rgb_ptr, d_mean_ptr=None, stream=None, rank=0, world=1,
                        tiled=False, want_stats=True, width=None, height=None):
        """Enqueues a render whose outputs stay in device memory (raw device pointers)."""
        self._handle("run_view_device")
        cam = self._cam(eye_pos, inv_view_mat, fovY)
        prm = self._device_params(rank, world, tiled, width, height)
        st = capi.Stats()
        capi.check(capi.lib().crt_render_device(self._h, C.byref(cam), C.byref(prm), C.c_void_p(d_rgb_ptr),
                                                C.c_void_p(d_mean_ptr) if d_mean_ptr else None,
                                                C.c_void_p(stream) if stream else None,
                                                C.byref(st) if want_stats else None), "crt_render_device")
        if want_stats:
            self.stats = st.as_dict()
        return self.stats

    def _aov_host(self, fn, view, width, height, groups, info_attr, sp=None):
        """The host form `fn` of an AOV pass for view = (eye_pos, inv_view_mat, fovY).  groups: per buffer struct of the C call, in its
        order, (names wanted, buffer table, ctypes struct, pass NULL when no name is given); sp: the settings struct of the forms that
        take one (AovSpecularParams, AovAoParams).  Returns {name: zeroed array the pass has filled}; self.<info_attr> gets the crt_aov_info dict."""
        h_ = self._handle("run_view" + fn[len("crt_render"):])
        cam = self._cam(*view)
        prm = self._params(flags=self.extra_flags, width=width, height=height)
        w, h = prm.width, prm.height
        out, structs = {}, []
        for names, table, struct, null_if_empty in groups:
            bufs = struct()
            for name in names:
                ch, dt = table[name]
                out[name] = np.zeros((h, w, 3) if ch == 3 else (h, w), dtype=dt)
                setattr(bufs, name, out[name].ctypes.data)
            structs.append(None if (null_if_empty and not names) else C.byref(bufs))
        info = capi.AovInfo()
        capi.check(getattr(capi.lib(), fn)(h_, C.byref(cam), C.byref(prm), *([C.byref(sp)] if sp else []), *structs, C.byref(info)), fn)
        setattr(self, info_attr, info.as_dict())
        return out

    def _aov_device(self, fn, view, shard, groups, info_attr, stream, want_info, sp=None, kind="AOV"):
        """The device form `fn` of an AOV pass for view = (eye_pos, inv_view_mat, fovY) and shard = (rank, world, tiled, width, height).
        groups as _aov_host's, with {name: raw device pointer} (or None) for the names; kind: what an unknown name is called.  With
        want_info sets and returns self.<info_attr>."""
        h_ = self._handle("run_view" + fn[len("crt_render"):])
        cam = self._cam(*view)
        prm = self._device_params(*shard)
        structs = []
        for ptrs, table, struct, null_if_empty in groups:
            bufs = struct()
            for name, p in (ptrs or {}).items():
                if name not in table:
                    raise ValueError("unknown %s buffer %r" % (kind, name))
                setattr(bufs, name, int(p) if p else None)
            structs.append(None if (null_if_empty and not ptrs) else C.byref(bufs))
        info = capi.AovInfo()
        capi.check(getattr(capi.lib(), fn)(h_, C.byref(cam), C.byref(prm), *([C.byref(sp)] if sp else []), *structs,
                                           C.c_void_p(stream) if stream else None, C.byref(info) if want_info else None), fn)
        if want_info:
            setattr(self, info_attr, info.as_dict())
        return getattr(self, info_attr) if want_info else None

    def run_view_aov(self, eye_pos, inv_view_mat, fovY, want=tuple(capi.AOV_BUFFERS), width=None, height=None):
        """First-hit AOVs of the frame run_view draws with the same camera and settings (crt_render_aov): per pixel, the spp camera
        rays of the frame's paths traced for their closest hit.  Returns {name: array} for the names in `want` (albedo, normal:
        (H, W, 3) float32; depth, coverage: (H, W) float32; tri, material: (H, W) int32); self.aov_info gets rays, chunks, total_ms."""
        return self._aov_host("crt_render_aov", (eye_pos, inv_view_mat, fovY), width, height, [(want, capi.AOV_BUFFERS, capi.AovBuffers, False)], "aov_info")

    def run_view_aov_device(self, eye_pos, inv_view_mat, fovY, ptrs, stream=None, rank=0, world=1, tiled=False, want_info=True,
                            width=None, height=None):
        """Enqueues the AOV pass with outputs in device memory: ptrs = {name: raw device pointer} (row-major W x H, or the shard's
        compact tiles with tiled / world > 1, as run_view_device).  With want_info the call synchronizes the stream and sets
        self.aov_info."""
        return self._aov_device("crt_render_aov_device", (eye_pos, inv_view_mat, fovY), (rank, world, tiled, width, height),
                                [(ptrs, capi.AOV_BUFFERS, capi.AovBuffers, False)], "aov_info", stream, want_info)

    def run_view_aov_shading(self, eye_pos, inv_view_mat, fovY, want=tuple(capi.AOV_SHADING_BUFFERS), first=(), width=None, height=None):
        """Shading AOVs (crt_render_aov_shading, contract: include/crt.h): emission -- ke / spp over the samples whose camera ray hits
        an emitter -- and diffuse_albedo -- kd / spp over the other hits --, what demodulate() takes.  `first` names buffers of
        run_view_aov to fill from the same trace (crt_render_aov's bits).  Returns {name: array} for the names in `want` and `first`;
        self.aov_info gets rays, chunks, total_ms."""
        out = self._aov_host("crt_render_aov_shading", (eye_pos, inv_view_mat, fovY), width, height,
                             [(first, capi.AOV_BUFFERS, capi.AovBuffers, True), (want, capi.AOV_SHADING_BUFFERS, capi.AovShadingBuffers, False)], "aov_info")
        return {name: out[name] for name in (*want, *first)}

    def run_view_aov_shading_device(self, eye_pos, inv_view_mat, fovY, ptrs, first_ptrs=None, stream=None, rank=0, world=1, tiled=False,
                                    want_info=True, width=None, height=None):
        """The same with outputs in device memory: ptrs = {"emission" / "diffuse_albedo": raw device pointer}, first_ptrs the same for
        buffers of run_view_aov_device (None: none); layout, stream and want_info as run_view_aov_device."""
        return self._aov_device("crt_render_aov_shading_device", (eye_pos, inv_view_mat, fovY), (rank, world, tiled, width, height),
                                [(first_ptrs, capi.AOV_BUFFERS, capi.AovBuffers, True), (ptrs, capi.AOV_SHADING_BUFFERS, capi.AovShadingBuffers, False)],
                                "aov_info", stream, want_info)

    def run_view_aov_direct(self, eye_pos, inv_view_mat, fovY, want=tuple(capi.AOV_DIRECT_BUFFERS), width=None, height=None):
        """Direct-light AOVs (crt_render_aov_direct, contract: include/crt.h): the first-vertex next-event term of the very paths
        run_view traces with the same camera and settings, recomputed sample for sample.  Returns {name: array} for the names in `want`
        (direct, unshadowed, direct_variance: (H, W, 3) float32; visibility: (H, W) float32).  light_sample_n is the frame's; p_rr is
        not read.  self.aov_direct_info gets rays (camera and traced shadow rays), chunks (sub-batches), total_ms."""
        return self._aov_host("crt_render_aov_direct", (eye_pos, inv_view_mat, fovY), width, height,
                              [(want, capi.AOV_DIRECT_BUFFERS, capi.AovDirectBuffers, False)], "aov_direct_info")

    def run_view_aov_direct_device(self, eye_pos, inv_view_mat, fovY, ptrs, stream=None, rank=0, world=1, tiled=False, want_info=True,
                                   width=None, height=None):
        """The same with outputs in device memory: ptrs = {name: raw device pointer}, layout as run_view_aov_device.  The call
        synchronizes the stream once per sub-batch (and once more with want_info, which sets self.aov_direct_info)."""
        return self._aov_device("crt_render_aov_direct_device", (eye_pos, inv_view_mat, fovY), (rank, world, tiled, width, height),
                                [(ptrs, capi.AOV_DIRECT_BUFFERS, capi.AovDirectBuffers, False)], "aov_direct_info", stream, want_info,
                                kind="direct-light AOV")

    def aov_ao_defaults(self):
        """crt_aov_ao_defaults of this scene as a dict: ao_samples 4, max_distance a quarter of the diagonal of the scene's root box.
        Both are tuned on nothing."""
        p = capi.AovAoParams()
        capi.check(capi.lib().crt_aov_ao_defaults(self._handle("aov_ao_defaults"), C.byref(p)), "crt_aov_ao_defaults")
        return {"ao_samples": int(p.ao_samples), "max_distance": float(p.max_distance)}

    def _aov_ao_params(self, ao_samples, max_distance):
        d = self.aov_ao_defaults()
        return capi.AovAoParams(d["ao_samples"] if ao_samples is None else int(ao_samples), d["max_distance"] if max_distance is None else float(max_distance))

    def run_view_aov_ao(self, eye_pos, inv_view_mat, fovY, ao_samples=None, max_distance=None, want=tuple(capi.AOV_AO_BUFFERS), width=None, height=None):
        """Ambient-occlusion AOVs (crt_render_aov_ao, contract: include/crt.h): per camera ray's hit, ao_samples rays of at most
        max_distance over the hemisphere of the facing normal.  Returns {name: array} for the names in `want` (ao, openness: (H, W)
        float32; bent_normal: (H, W, 3) float32).  None: aov_ao_defaults'.  p_rr and light_sample_n are not read.  self.aov_ao_info
        gets rays (camera and occlusion rays), chunks (sub-batches), total_ms."""
        return self._aov_host("crt_render_aov_ao", (eye_pos, inv_view_mat, fovY), width, height,
                              [(want, capi.AOV_AO_BUFFERS, capi.AovAoBuffers, False)], "aov_ao_info", sp=self._aov_ao_params(ao_samples, max_distance))

    def run_view_aov_ao_device(self, eye_pos, inv_view_mat, fovY, ptrs, ao_samples=None, max_distance=None, stream=None, rank=0, world=1, tiled=False,
                               want_info=True, width=None, height=None):
        """The same with outputs in device memory: ptrs = {name: raw device pointer}, layout as run_view_aov_device.  The call only
        enqueues; with want_info it synchronizes the stream once, at the end, and sets self.aov_ao_info."""
        return self._aov_device("crt_render_aov_ao_device", (eye_pos, inv_view_mat, fovY), (rank, world, tiled, width, height),
                                [(ptrs, capi.AOV_AO_BUFFERS, capi.AovAoBuffers, False)], "aov_ao_info", stream, want_info,
                                sp=self._aov_ao_params(ao_samples, max_distance), kind="ambient-occlusion AOV")

    def run_view_aov_specular(self, eye_pos, inv_view_mat, fovY, max_bounces=None, want=tuple(capi.AOV_SPECULAR_BUFFERS), width=None, height=None):
        """AOVs that follow perfect-mirror bounces from the first hit (crt_render_aov_specular, contract: include/crt.h): returns
        {name: array} for the names in `want` (guide_albedo, last_normal: (H, W, 3) float32; path_depth, bounces: (H, W) float32;
        last_tri: (H, W) int32).  max_bounces None: crt_aov_specular_defaults'.  self.aov_specular_info gets rays (camera and
        reflected), chunks, total_ms."""
        return self._aov_host("crt_render_aov_specular", (eye_pos, inv_view_mat, fovY), width, height,
                              [(want, capi.AOV_SPECULAR_BUFFERS, capi.AovSpecularBuffers, False)], "aov_specular_info", sp=_aov_specular_params(max_bounces))

    def run_view_aov_specular_device(self, eye_pos, inv_view_mat, fovY, ptrs, max_bounces=None, stream=None, rank=0, world=1, tiled=False,
                                     want_info=True, width=None, height=None):
        """The same with outputs in device memory: ptrs = {name: raw device pointer}, layout as run_view_aov_device.  The call
        synchronizes the stream once per bounce and chunk (and once more with want_info, which sets self.aov_specular_info)."""
        return self._aov_device("crt_render_aov_specular_device", (eye_pos, inv_view_mat, fovY), (rank, world, tiled, width, height),
                                [(ptrs, capi.AOV_SPECULAR_BUFFERS, capi.AovSpecularBuffers, False)], "aov_specular_info", stream, want_info,
                                sp=_aov_specular_params(max_bounces), kind="specular AOV")

    def run_view_denoised(self, eye_pos, inv_view_mat, fovY, iterations=None, sigma_color=None, sigma_normal=None, sigma_albedo=None,
                          sigma_depth=None, width=None, height=None, variance_guided=False, specular_guides=False, max_bounces=None,
                          demodulate=False, albedo_floor=None, nlm=None, regress=None, scales=None, split_direct=False):
        """The frame of run_view, filtered by the AOV-guided a-trous denoiser (crt_denoise) with the albedo, normal and depth of
        run_view_aov as guides: returns (rgb (H, W, 3) uint8, mean (H, W, 3) float32) of the denoised frame.  The noisy frame stays in
        self.frame_buffer / self.mean_buffer, the guides in self.aov_buffers, the filter's timer in self.denoise_info.
        variance_guided: render with want_variance and filter with crt_denoise_var (its own defaults) and self.variance_buffer.
        nlm: True, or a dict of denoise_nlm's settings (radius, patch, k, alpha): render with want_variance and filter with crt_denoise_nlm
        instead of the a-trous filter; the sigma_normal, sigma_albedo and sigma_depth arguments go to it.  It composes with specular_guides
        and demodulate as variance_guided does, and excludes variance_guided, iterations and sigma_color (ValueError).
        regress: True, or a dict of denoise_regress's settings: render with want_variance and filter with crt_denoise_regress; composes
        and excludes as nlm does, and excludes nlm.  The sigma arguments scale its features.  With demodulate the albedo feature is
        dropped from the mask: irradiance does not follow the albedo.  self.denoise_info then holds total_ms and fallback_pixels.
        specular_guides: the albedo guide is guide_albedo of run_view_aov_specular (max_bounces) -- what a mirror reflects instead of the
        mirror; normal and depth stay first-hit.
        demodulate: the filter runs on irradiance.  The shading AOVs (self.shading_buffers: emission, diffuse_albedo) come from the same
        pass as the guides, the frame (and, variance_guided, its variance) goes through demodulate(albedo_floor), is filtered with the
        caller's sigmas -- the albedo guide is still passed; sigma_albedo=float("inf") drops it -- and comes back through modulate().
        scales: None or 1 is the single filter call; 2 .. 4 runs the filter as denoise_multiscale does, a Laplacian pyramid of that many
        scales with the same settings at each, where the single call stands (so it composes with demodulate and specular_guides).  It
        needs variance_guided, nlm or regress (ValueError); self.denoise_info is then denoise_multiscale's dict.
        split_direct: direct and indirect light are filtered separately (SVGF's split) -- `direct` of run_view_aov_direct, with its
        direct_variance, and mean - direct, with the frame's variance (which overstates it), through the same filter with the same
        settings; the two results are added (crt_modulate with a zero albedo: a + b, and the frame's tone map).  With the plain and the
        variance-guided filter, one scale, no demodulate (ValueError otherwise).  self.direct_buffers keeps direct and direct_variance,
        self.denoise_info the info of the indirect part's call."""
        self._handle("run_view_denoised")
        name, settings, scales = _denoise_request("run_view_denoised", variance_guided, iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth,
                                                  nlm, regress, scales, demodulate)
        with_variance = _FILTERS[name][2]
        if split_direct and (name not in ("atrous", "var") or scales > 1 or demodulate):
            raise ValueError("run_view_denoised: split_direct works with the plain and the variance-guided filter at one scale, without demodulate")
        self.run_view(eye_pos, inv_view_mat, fovY, width=width, height=height, want_variance=with_variance)
        guides = ("albedo", "normal", "depth")
        if demodulate:
            aov = self.run_view_aov_shading(eye_pos, inv_view_mat, fovY, first=guides, width=width, height=height)
            self.aov_buffers = {k: aov[k] for k in guides}
            self.shading_buffers = {k: aov[k] for k in capi.AOV_SHADING_BUFFERS}
        else:
            self.aov_buffers = self.run_view_aov(eye_pos, inv_view_mat, fovY, want=guides, width=width, height=height)
        if specular_guides:
            self.aov_buffers["albedo"] = self.run_view_aov_specular(eye_pos, inv_view_mat, fovY, max_bounces=max_bounces, want=("guide_albedo",),
                                                                    width=width, height=height)["guide_albedo"]
        if split_direct:
            self.direct_buffers = self.run_view_aov_direct(eye_pos, inv_view_mat, fovY, want=("direct", "direct_variance"), width=width, height=height)
            direct, dvar = self.direct_buffers["direct"], self.direct_buffers["direct_variance"]
            a = _run_filter(name, direct, dvar if with_variance else None, self.aov_buffers, settings, self.device, False)[1]
            _, b, self.denoise_info = _run_filter(name, self.mean_buffer - direct, self.variance_buffer if with_variance else None, self.aov_buffers,
                                                  settings, self.device, False)
            return _modulate(a, np.zeros_like(a), b, device=self.device)
        return self._filter_frame(name, settings, scales, demodulate, albedo_floor)

    def _filter_frame(self, name, settings, scales, demodulate, albedo_floor):
        """What run_view_denoised -- and MultiRender.run_view_gathered_denoised -- does once the frame's buffers exist: filter `name` of
        _FILTERS with `settings` on self.mean_buffer (and self.variance_buffer) with the guides in self.aov_buffers, at `scales` scales,
        between demodulate() and modulate() with self.shading_buffers when `demodulate`.  Returns (rgb, mean); sets self.denoise_info."""
        with_variance = _FILTERS[name][2]
        color, var = self.mean_buffer, self.variance_buffer if with_variance else None
        if demodulate:
            sh = self.shading_buffers
            got = _demodulate(color, sh["diffuse_albedo"], sh["emission"], variance=var, albedo_floor=albedo_floor, device=self.device)
            color, var = got if with_variance else (got, None)
        if scales > 1:
            rgb, mean, self.denoise_info = denoise_multiscale(color, var, filter=name, scales=scales, device=self.device, want_rgb=not demodulate,
                                                              return_info=True, **settings, **self.aov_buffers)
        else:
            rgb, mean, self.denoise_info = _run_filter(name, color, var, self.aov_buffers, settings, self.device, not demodulate)
        if demodulate:
            rgb, mean = _modulate(mean, sh["diffuse_albedo"], sh["emission"], albedo_floor=albedo_floor, device=self.device)
        return rgb, mean

    def run_view_selected(self, eye_pos, inv_view_mat, fovY, candidates=("var", "nlm"), error_radius=None, blend_radius=None, width=None, height=None):
        """The frame of run_view with, per pixel, the one of the candidate filters whose error estimated against the independent other
        half frame is smallest (crt_filter_select, contract: include/crt.h).  Renders with want_halves, takes the guides of run_view_aov,
        runs every candidate on each half -- "none" (the half as it is), "atrous" (denoise), "var" (denoise_var) or "nlm" (denoise_nlm),
        each with its own defaults; the variance-taking ones get 2 x the frame's variance, the variance of one half's mean -- and calls
        filter_select.  "reg" (denoise_regress) filters each half with weights from the OTHER half (weight_color; weight_variance is the
        half variance), so that a half's weights do not follow its own noise.  Returns (rgb (H, W, 3) uint8, mean (H, W, 3) float32).
        Kept: the noisy frame in self.frame_buffer / self.mean_buffer, the guides in self.aov_buffers, self.select_buffers (choice (H, W) uint8, error (H, W) float32, half_a, half_b,
        half_variance, filtered_a, filtered_b) and self.select_info (total_ms, chosen)."""
        names = _select_request("run_view_selected", candidates)
        self._handle("run_view_selected")
        self.run_view(eye_pos, inv_view_mat, fovY, width=width, height=height, want_halves=True)
        self.aov_buffers = self.run_view_aov(eye_pos, inv_view_mat, fovY, want=("albedo", "normal", "depth"), width=width, height=height)
        return self._select_frame(names, error_radius, blend_radius)

    def _select_frame(self, names, error_radius, blend_radius):
        """What run_view_selected -- and MultiRender.run_view_gathered_selected -- does once the halves (self.half_a_buffer,
        self.half_b_buffer), the frame's variance and the guides in self.aov_buffers exist: the candidates `names` on each half, then
        filter_select.  Returns (rgb, mean); sets self.select_buffers and self.select_info."""
        guides = self.aov_buffers
        a, b = self.half_a_buffer, self.half_b_buffer
        half_var = np.float32(2.0) * self.variance_buffer
        fa = [_select_candidate(n, a, half_var, guides, self.device, other=b) for n in names]
        fb = [_select_candidate(n, b, half_var, guides, self.device, other=a) for n in names]
        rgb, mean, choice, error, self.select_info = filter_select(a, b, half_var, fa, fb, error_radius=error_radius, blend_radius=blend_radius,
                                                                   device=self.device, return_info=True)
        self.select_buffers = {"choice": choice, "error": error, "half_a": a, "half_b": b, "half_variance": half_var, "filtered_a": fa, "filtered_b": fb}
        return rgb, mean

    def run_view_upsampled(self, eye_pos, inv_view_mat, fovY, factor=2, width=None, height=None, guide_spp=None, demodulate=True, filter_low=False,
                           albedo_floor=None, **upsample_settings):
        """Resolution scaling: the frame's paths at (W / factor, H / factor), its first hits at (W, H), and crt_upsample in between
        (contract: include/crt.h).  Renders the low-resolution frame with want_variance, runs the shading AOV pass with albedo, normal and
        depth at the low size and again at the full size -- there with guide_spp samples per pixel (None: self.spp; self.spp is what it was
        afterwards) --, upsamples the low frame along the two sets of guides and returns (rgb (H, W, 3) uint8, mean (H, W, 3) float32).
        demodulate (the default): what is upsampled is irradiance -- the low frame and its variance through demodulate(albedo_floor) with
        the LOW shading AOVs, the result through modulate() with the FULL-resolution ones, so texture and the edges of emitters come from
        the full-resolution pass; False: the radiance itself is upsampled.  filter_low: denoise_var (its defaults) on the low image first;
        the variance that is upsampled is then still the unfiltered frame's and overstates what is left.  upsample_settings: radius,
        min_weight, sigma_normal, sigma_albedo, sigma_depth of upsample().  factor is 2 .. 8 and must divide both sides (ValueError).
        Kept: self.low_frame (rgb, mean, variance and the AOVs of the low frame), self.aov_buffers and self.shading_buffers (full
        resolution), self.upsampled_variance (of what was upsampled: irradiance with demodulate), self.upsample_info."""
        w, h = width or self.scene.width, height or self.scene.height
        if factor != int(factor) or not 2 <= int(factor) <= 8:
            raise ValueError("run_view_upsampled: factor must be an integer 2 .. 8, got %r" % (factor,))
        factor = int(factor)
        if w % factor or h % factor:
            raise ValueError("run_view_upsampled: %d x %d is not divisible by the factor %d" % (w, h, factor))
        self._handle("run_view_upsampled")
        lw, lh = w // factor, h // factor
        view, guides = (eye_pos, inv_view_mat, fovY), ("albedo", "normal", "depth")
        low_rgb = self.run_view(*view, width=lw, height=lh, want_variance=True)
        low = dict(self.run_view_aov_shading(*view, first=guides, width=lw, height=lh), rgb=low_rgb, mean=self.mean_buffer, variance=self.variance_buffer)
        spp = self.spp
        try:
            if guide_spp is not None:
                self.set_spp(guide_spp)
            full = self.run_view_aov_shading(*view, first=guides, width=w, height=h)
        finally:
            self.spp = spp
        self.low_frame = low
        self.aov_buffers = {k: full[k] for k in guides}
        self.shading_buffers = {k: full[k] for k in capi.AOV_SHADING_BUFFERS}
        color, var = low["mean"], low["variance"]
        if demodulate:
            color, var = _demodulate(color, low["diffuse_albedo"], low["emission"], variance=var, albedo_floor=albedo_floor, device=self.device)
        low_guides = {k: low[k] for k in guides}
        if filter_low:
            color = _run_filter("var", color, var, low_guides, {}, self.device, False)[1]
        rgb, mean, self.upsampled_variance, self.upsample_info = upsample(dict(low_guides, color=color, variance=var), w, h, guides=self.aov_buffers,
                                                                          device=self.device, want_rgb=not demodulate, return_info=True,
                                                                          **upsample_settings)
        if demodulate:
            rgb, mean = _modulate(mean, full["diffuse_albedo"], full["emission"], albedo_floor=albedo_floor, device=self.device)
        return rgb, mean

    def run_view_temporal(self, eye_pos, inv_view_mat, fovY, denoise=False, seed=None, width=None, height=None, clamp=None, variance="samples",
                          demodulate=False, albedo_floor=None, specular=False, **overrides):
        """One frame of a temporally accumulated sequence (crt_temporal, contract: include/crt.h): renders with want_variance, runs the
        AOV pass (albedo, normal, depth, material) and blends the frame into the history this object keeps -- colour, variance, history
        length, depth, normal, material ID and camera of the previous call; the unfiltered result is the next call's history.
        Returns (rgb, mean) of the accumulated frame, or with denoise=True of its variance-guided filter (denoise_var of the accumulated
        mean and variance, the frame's guides).  seed=None renders with self.seed + the number of frames since the last reset (the
        frames must not share a seed); overrides: depth_tolerance, normal_tolerance, alpha_min; clamp: temporal()'s (None: the history is
        not clamped; self.temporal_info then has no `clamped`).  The first call, the first after
        reset_temporal() and the first at another size start a history.  self.frame_buffer / self.mean_buffer hold the frame as
        rendered, self.variance_buffer the accumulated variance, self.temporal_history_buffer the frames accumulated per pixel (H, W),
        self.temporal_info the crt_temporal_info dict, self.aov_buffers the guides.
        variance="moments": the frame is rendered WITHOUT want_variance (so one sample per pixel works), the history also keeps the
        moment planes of crt_temporal_moments, and self.variance_buffer -- what denoise=True feeds to denoise_var -- is
        variance_estimate of them with the frame's normal and depth; overrides may then also name variance_estimate's settings, and
        self.variance_estimate_info holds its info dict.  A change of `variance` starts a history.
        demodulate: the sequence is accumulated as irradiance.  Each frame's shading AOVs (self.shading_buffers) come from the pass of
        its guides; the frame and its variance go through demodulate(albedo_floor) before the blend, so the history -- and with it the
        clamp's neighbourhood, the moments and self.variance_buffer -- holds irradiance and its variance.  What is returned (and, with
        denoise=True, filtered first, on irradiance) goes through modulate() with the CURRENT frame's buffers.  A change of `demodulate`
        starts a history.
        specular: False, True or a dict of max_bounces / radius / min_bounces -- crt_temporal_dual: each frame also runs
        run_view_aov_specular (max_bounces), its path_depth, bounces and last_normal are kept with the history, and a mirror pixel also
        tries the history its virtual image points at (temporal(dual=dict(radius=, min_bounces=))); self.temporal_info gains `clamped`
        (0 without a clamp), `virtual_tried` and `virtual_taken`.  It composes with clamp, denoise and demodulate and excludes
        variance="moments" (ValueError).  A change of `specular` between False and not starts a history."""
        if variance not in ("samples", "moments"):
            raise ValueError("run_view_temporal: variance must be 'samples' or 'moments', got %r" % (variance,))
        dual = max_bounces = None
        if specular is not False:
            if specular is not True and (not isinstance(specular, dict) or set(specular) - {"max_bounces", "radius", "min_bounces"}):
                raise ValueError("run_view_temporal: specular must be False, True or a dict of max_bounces / radius / min_bounces, got %r" % (specular,))
            if variance == "moments":
                raise ValueError("run_view_temporal: specular and variance='moments' cannot be combined (crt_temporal_moments has no dual form)")
            settings = {} if specular is True else specular
            max_bounces = settings.get("max_bounces")
            dual = {k: settings[k] for k in ("radius", "min_bounces") if k in settings} or True
        self._handle("run_view_temporal")
        demodulate = bool(demodulate)
        if self._temporal is not None and self._temporal.get("demodulate", False) != demodulate:
            self._temporal = None
        if self._temporal is not None and ("path_depth" in self._temporal["prev"]) != (dual is not None):
            self._temporal = None
        if variance == "moments":
            return self._run_view_temporal_moments(eye_pos, inv_view_mat, fovY, denoise, seed, width, height, clamp, overrides, demodulate, albedo_floor)
        if self._temporal is not None and "m1" in self._temporal:
            self._temporal = None
        aov = self._temporal_frame(eye_pos, inv_view_mat, fovY, seed, width, height, True, demodulate, specular=(max_bounces,) if dual is not None else None)
        h, w = self.mean_buffer.shape[:2]
        cam = (np.array(eye_pos, dtype=np.float32), np.array(inv_view_mat, dtype=np.float32).reshape(9), np.float32(fovY))
        cur = {"color": self.mean_buffer, "variance": self.variance_buffer, "depth": aov["depth"], "normal": aov["normal"], "id": aov["material"]}
        if demodulate:
            sh = self.shading_buffers
            cur["color"], cur["variance"] = _demodulate(self.mean_buffer, sh["diffuse_albedo"], sh["emission"], variance=self.variance_buffer,
                                                        albedo_floor=albedo_floor, device=self.device)
        if dual is not None:
            cur.update({k: aov[k] for k in _SPECULAR_PLANES})
            overrides = dict(overrides, dual=dual)
        t = self._temporal if (self._temporal is not None and self._temporal["size"] == (w, h)) else None
        rgb, mean, var, hist, info = temporal(cur, cam, prev=t["prev"] if t else None, prev_camera=t["camera"] if t else None, device=self.device,
                                              return_info=True, clamp=clamp, want_rgb=not demodulate, **overrides)
        self._temporal = {"prev": dict(cur, color=mean, variance=var, history=hist), "camera": cam, "size": (w, h), "demodulate": demodulate}
        self._temporal_frames += 1
        self.variance_buffer, self.temporal_history_buffer, self.temporal_info = var, hist, info
        return self._temporal_result(rgb, mean, var, denoise, demodulate, albedo_floor)

    def _temporal_frame(self, eye_pos, inv_view_mat, fovY, seed, width, height, want_variance, demodulate, specular=None):
        """Renders a frame of run_view_temporal with its seed and runs the pass of its guides (self.aov_buffers) and, demodulate, of its
        shading AOVs (self.shading_buffers); returns the first-hit buffers the blend takes.  specular: None or (max_bounces,) -- the
        specular AOV pass runs with the frame's seed too, and its three planes are returned with the others."""
        names = ("albedo", "normal", "depth", "material")
        keep_seed = self.seed
        self.seed = keep_seed + self._temporal_frames if seed is None else int(seed)
        try:
            self.run_view(eye_pos, inv_view_mat, fovY, width=width, height=height, want_variance=want_variance)
            if demodulate:
                aov = self.run_view_aov_shading(eye_pos, inv_view_mat, fovY, first=names, width=width, height=height)
                self.shading_buffers = {k: aov[k] for k in capi.AOV_SHADING_BUFFERS}
            else:
                aov = self.run_view_aov(eye_pos, inv_view_mat, fovY, want=names, width=width, height=height)
            if specular is not None:
                aov = dict(aov, **self.run_view_aov_specular(eye_pos, inv_view_mat, fovY, max_bounces=specular[0], want=_SPECULAR_PLANES, width=width,
                                                             height=height))
        finally:
            self.seed = keep_seed
        self.aov_buffers = {k: aov[k] for k in ("albedo", "normal", "depth")}
        return aov

    def _temporal_result(self, rgb, mean, var, denoise, demodulate, albedo_floor):
        """What run_view_temporal returns of the accumulated frame (mean, var): filtered with denoise, and back from irradiance with
        demodulate."""
        if denoise:
            rgb, mean, self.denoise_info = _run_filter("var", mean, var, self.aov_buffers, {}, self.device, not demodulate)
        if demodulate:
            sh = self.shading_buffers
            rgb, mean = _modulate(mean, sh["diffuse_albedo"], sh["emission"], albedo_floor=albedo_floor, device=self.device)
        return rgb, mean

    def _run_view_temporal_moments(self, eye_pos, inv_view_mat, fovY, denoise, seed, width, height, clamp, overrides, demodulate=False, albedo_floor=None):
        estimate = {k: overrides.pop(k) for k in list(overrides) if k in _ESTIMATE_SETTINGS}
        aov = self._temporal_frame(eye_pos, inv_view_mat, fovY, seed, width, height, False, demodulate)
        h, w = self.mean_buffer.shape[:2]
        cam = (np.array(eye_pos, dtype=np.float32), np.array(inv_view_mat, dtype=np.float32).reshape(9), np.float32(fovY))
        cur = {"color": self.mean_buffer, "depth": aov["depth"], "normal": aov["normal"], "id": aov["material"]}
        if demodulate:
            sh = self.shading_buffers
            cur["color"] = _demodulate(self.mean_buffer, sh["diffuse_albedo"], sh["emission"], albedo_floor=albedo_floor, device=self.device)
        t = self._temporal if (self._temporal is not None and self._temporal["size"] == (w, h) and "m1" in self._temporal) else None
        rgb, mean, _, hist, m1, m2, info = temporal(cur, cam, prev=t["prev"] if t else None, prev_camera=t["camera"] if t else None, device=self.device,
                                                    return_info=True, clamp=clamp, moments={"m1": t["m1"], "m2": t["m2"]} if t else True,
                                                    want_rgb=not demodulate, **overrides)
        self._temporal = {"prev": dict(cur, color=mean, history=hist), "camera": cam, "size": (w, h), "m1": m1, "m2": m2, "demodulate": demodulate}
        self._temporal_frames += 1
        var, self.variance_estimate_info = variance_estimate(m1, m2, hist, normal=aov["normal"], depth=aov["depth"], device=self.device,
                                                             return_info=True, **estimate)
        self.variance_buffer, self.temporal_history_buffer, self.temporal_info = var, hist, info
        return self._temporal_result(rgb, mean, var, denoise, demodulate, albedo_floor)

    def reset_temporal(self):
        """Drops the history of run_view_temporal: the next call is a first frame (and renders with self.seed again)."""
        self._temporal = None
        self._temporal_frames = 0

    def intersect(self, origins, dirs, traversal=None):
        self._handle("intersect")
        o = np.ascontiguousarray(origins, dtype=np.float32)
        d = np.ascontiguousarray(dirs, dtype=np.float32)
        n = o.shape[0]
        tri = np.zeros(n, dtype=np.int32)
        t = np.zeros(n, dtype=np.float32)
        capi.check(capi.lib().crt_intersect(self._h, n, capi.ptr(o), capi.ptr(d),
                                            self.traversal if traversal is None else traversal, capi.ptr(tri),
                                            capi.ptr(t)), "crt_intersect")
        return tri, t

    def blocked(self, origins, dirs, limits, traversal=None):
        """blocked() of Render.cuh:19-27 for n visibility rays with t_to_light = limits: (blocked, blocking triangle or -1)"""
        self._handle("blocked")
        o = np.ascontiguousarray(origins, dtype=np.float32)
        d = np.ascontiguousarray(dirs, dtype=np.float32)
        n = o.shape[0]
        tri = np.zeros(n, dtype=np.int32)
        t = np.array(limits, dtype=np.float32).reshape(n).copy()
        capi.check(capi.lib().crt_intersect(self._h, n, capi.ptr(o), capi.ptr(d),
                                            (self.traversal if traversal is None else traversal) | capi.INTERSECT_VISIBILITY,
                                            capi.ptr(tri), capi.ptr(t)), "crt_intersect")
        return t != 0.0, tri

    def save_frame_buffer(self, save_path):
        if self.frame_buffer is None:
            raise RuntimeError("save_frame_buffer before run_view")
        h, w, _ = self.frame_buffer.shape
        capi.check(capi.lib().crt_write_png(os.fsencode(save_path), w, h, capi.ptr(self.frame_buffer)), "crt_write_png")

    def get_frame_buffer(self):
        return self.frame_buffer

    def free(self):
        if self._h:
            capi.lib().crt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MultiRender(Render):
    """Render over several devices of one node in ONE process (include/crt.h, crt_multi): one replica of the scene per entry
    of `devices`, interleaved pixel-tile shards, one RCCL all-gather per frame.  The reference stops at device 0
    (src/main.cu:92-105)."""

    def __init__(self, scene, spp=16, P_RR=0.8, light_sample_n=1, devices=(0,), gather=capi.GATHER_AUTO):
        self.scene = scene
        self.spp, self.P_RR, self.light_sample_n = int(spp), np.float32(P_RR), int(light_sample_n)
        self.seed = 0
        self.traversal = capi.TRAVERSAL_EXACT
        self.extra_flags = 0
        self.devices = [int(d) for d in devices]
        self.device = self.devices[0]
        self._h = C.c_void_p()   # stays null: every inherited method that takes a crt_scene* fails its own check
        self._mh = C.c_void_p()  # the crt_multi*
        devs = (C.c_int * len(self.devices))(*self.devices)
        capi.check(capi.lib().crt_multi_create(C.byref(scene.desc()), devs, len(self.devices), gather, C.byref(self._mh)),
                   "crt_multi_create")
        self.frame_buffer = None
        self.mean_buffer = None
        self.stats = None
        self.rank_stats = None
        self.info = None
        # run_view_gathered and its filtered forms: as Render's
        self.variance_buffer = self.half_a_buffer = self.half_b_buffer = None
        self.aov_buffers = self.shading_buffers = None
        self.denoise_info = self.select_buffers = self.select_info = None

    def run_view(self, eye_pos, inv_view_mat, fovY, stats=False, want_mean=True, width=None, height=None, to_host=True, want_variance=False,
                 want_halves=False):
        if want_variance:
            raise NotImplementedError("the variance buffer is a single-device interface (crt_variance): there is no gather for it")
        if want_halves:
            raise NotImplementedError("the half buffers are a single-device interface (crt_half_buffers): there is no gather for them")
        if not self._mh:
            raise RuntimeError("MultiRender.run_view after free()")
        cam = self._cam(eye_pos, inv_view_mat, fovY)
        prm = self._params(flags=(capi.FLAG_STATS if stats else 0) | self.extra_flags, width=width, height=height)
        w, h = prm.width, prm.height
        rgb = np.zeros((h, w, 3), dtype=np.uint8) if to_host else None
        mean = np.zeros((h, w, 3), dtype=np.float32) if (want_mean and to_host) else None
        st = (capi.Stats * len(self.devices))()
        info = capi.MultiInfo()
        capi.check(capi.lib().crt_multi_render(self._mh, C.byref(cam), C.byref(prm), capi.ptr(rgb), capi.ptr(mean), st,
                                               C.byref(info)), "crt_multi_render")
        self._rank_totals(st, info)
        if to_host:
            self.frame_buffer, self.mean_buffer = rgb, mean
        return rgb

    def _rank_totals(self, st, info):
        """self.rank_stats, self.info and self.stats (the ranks' counters summed, their times' maximum) of a frame"""
        self.rank_stats = [s.as_dict() for s in st]
        self.info = info.as_dict()
        tot = dict(self.rank_stats[0])
        for o in self.rank_stats[1:]:
            for k in ("paths", "rays", "shadow_rays", "probe_rays", "rays_untraced", "inner_pops", "leaf_pops", "tri_tests", "hits"):
                tot[k] += o[k]
            for k in ("kernel_ms", "total_ms"):
                tot[k] = max(tot[k], o[k])
        self.stats = tot

    def run_view_gathered(self, eye_pos, inv_view_mat, fovY, want=("rgb", "mean", "variance", "albedo", "normal", "depth"), width=None, height=None,
                          to_host=True, stats=False):
        """The frame of run_view with the buffers the image filters take, gathered from all ranks (crt_multi_render_buffers, contract:
        include/crt.h).  want: names of capi.MULTI_BUFFERS -- rgb, mean, variance, half_a, half_b, the six of run_view_aov, emission,
        diffuse_albedo --; every plane has the bits of the single-device call it is named after.  Returns {name: array} ((H, W, 3) or
        (H, W), of the plane's type) and fills, as Render does, self.frame_buffer, self.mean_buffer, self.variance_buffer,
        self.half_a_buffer / self.half_b_buffer, self.aov_buffers and self.shading_buffers (dicts of the wanted names; None where nothing
        of the kind is wanted), self.info, self.rank_stats and self.stats.  to_host=False: nothing is copied and None is returned; the
        planes stay on rank 0's device (gathered_device()) and the host-side attributes are left as they were."""
        names = tuple(want)
        unknown = [n for n in names if n not in capi.MULTI_BUFFERS]
        if unknown:
            raise ValueError("run_view_gathered: unknown buffer(s) %r; the names are %r" % (unknown, tuple(capi.MULTI_BUFFERS)))
        if not self._mh:
            raise RuntimeError("MultiRender.run_view_gathered after free()")
        cam = self._cam(eye_pos, inv_view_mat, fovY)
        prm = self._params(flags=(capi.FLAG_STATS if stats else 0) | self.extra_flags, width=width, height=height)
        w, h = prm.width, prm.height
        mask, out, bufs = 0, {}, capi.MultiBuffers()
        for name in names:
            mask |= capi.MULTI_BITS[name]
            if to_host:
                ch, dt = capi.MULTI_BUFFERS[name]
                out[name] = np.zeros((h, w, 3) if ch == 3 else (h, w), dtype=dt)
                setattr(bufs, name, out[name].ctypes.data)
        st = (capi.Stats * len(self.devices))()
        info = capi.MultiInfo()
        capi.check(capi.lib().crt_multi_render_buffers(self._mh, C.byref(cam), C.byref(prm), mask, C.byref(bufs) if to_host else None, st, C.byref(info)),
                   "crt_multi_render_buffers")
        self._rank_totals(st, info)
        if not to_host:
            return None
        self.frame_buffer, self.mean_buffer, self.variance_buffer = out.get("rgb"), out.get("mean"), out.get("variance")
        self.half_a_buffer, self.half_b_buffer = out.get("half_a"), out.get("half_b")
        self.aov_buffers = {k: out[k] for k in capi.AOV_BUFFERS if k in out} or None
        self.shading_buffers = {k: out[k] for k in capi.AOV_SHADING_BUFFERS if k in out} or None
        return out

    def gathered_device(self):
        """({name: raw device pointer of the row-major plane, or None for a plane the last frame did not make}, device index) of the last
        frame on this handle (crt_multi_buffers_device) -- for the *_device forms of the filters, with no host round trip.  Valid until
        the next frame."""
        if not self._mh:
            raise RuntimeError("MultiRender.gathered_device after free()")
        bufs, dev = capi.MultiBuffers(), C.c_int(-1)
        capi.check(capi.lib().crt_multi_buffers_device(self._mh, C.byref(bufs), C.byref(dev)), "crt_multi_buffers_device")
        return {name: getattr(bufs, name) for name in capi.MULTI_BUFFERS}, dev.value

    def run_view_gathered_denoised(self, eye_pos, inv_view_mat, fovY, iterations=None, sigma_color=None, sigma_normal=None, sigma_albedo=None,
                                   sigma_depth=None, width=None, height=None, variance_guided=False, demodulate=False, albedo_floor=None, nlm=None,
                                   regress=None, scales=None):
        """Render.run_view_denoised on a frame rendered over all ranks: the arguments are its own (without specular_guides / max_bounces:
        there is no gather of the specular AOVs), the frame, its variance, the guides and -- demodulate -- the shading AOVs come from ONE
        run_view_gathered, and everything after that is the very function the single-device method runs on rank 0's device.  Returns
        (rgb, mean) with the single-device call's bits; the attributes are filled as there."""
        name, settings, scales = _denoise_request("run_view_gathered_denoised", variance_guided, iterations, sigma_color, sigma_normal, sigma_albedo,
                                                  sigma_depth, nlm, regress, scales, demodulate)
        want = ("rgb", "mean", "albedo", "normal", "depth") + (("variance",) if _FILTERS[name][2] else ()) + (tuple(capi.AOV_SHADING_BUFFERS) if demodulate else ())
        self.run_view_gathered(eye_pos, inv_view_mat, fovY, want=want, width=width, height=height)
        return self._filter_frame(name, settings, scales, demodulate, albedo_floor)

    def run_view_gathered_selected(self, eye_pos, inv_view_mat, fovY, candidates=("var", "nlm"), error_radius=None, blend_radius=None, width=None,
                                   height=None):
        """Render.run_view_selected on a frame rendered over all ranks: the halves, the variance and the guides come from ONE
        run_view_gathered, the candidates and filter_select are the very function the single-device method runs.  Returns (rgb, mean)
        with the single-device call's bits; self.select_buffers and self.select_info as there."""
        names = _select_request("run_view_gathered_selected", candidates)
        self.run_view_gathered(eye_pos, inv_view_mat, fovY, want=("rgb", "mean", "variance", "half_a", "half_b", "albedo", "normal", "depth"),
                               width=width, height=height)
        return self._select_frame(names, error_radius, blend_radius)

    def free(self):
        if self._mh:
            capi.lib().crt_multi_destroy(self._mh)
            self._mh = C.c_void_p()


# The single-device interfaces of Render that a MultiRender refuses, each with what it says
_MULTI_REFUSALS = {
    "run_view_range": "progressive ranges are a single-device interface (crt_render_range)",
    "run_view_adaptive": "adaptive sampling is a single-device interface (crt_render_adaptive)",
    "run_view_map": "sample maps are a single-device interface (crt_render_map)",
    "run_view_map_device": "sample maps are a single-device interface (crt_render_map_device)",
    "run_view_planned": "planned adaptive frames are a single-device interface (crt_render_planned)",
    "run_view_planned_device": "planned adaptive frames are a single-device interface (crt_render_planned_device)",
    "sample_plan": "the sample plan is a single-device interface (crt_sample_plan)",
    "frame_error": "the frame's error summary is a single-device interface (crt_frame_error)",
    "frame_error_device": "the frame's error summary is a single-device interface (crt_frame_error_device)",
    "run_view_until": "rendering to an error target is a single-device interface (crt_render_until)",
    "run_view_until_device": "rendering to an error target is a single-device interface (crt_render_until_device)",
    "preview": "previews are a single-device interface (crt_preview)",
    "variance": "the variance buffer is a single-device interface (crt_variance)",
    "half_buffers": "the half buffers are a single-device interface (crt_half_buffers)",
    "run_view_selected": "filter selection is a single-device interface (crt_half_buffers, crt_filter_select): gather the frame first",
    "accel_info": "crt_scene_accel_info is a single-device interface",
    "run_view_device": "MultiRender owns its device buffers (crt_multi_frame_device)",
    "run_view_aov": "the AOV pass is a single-device interface (crt_render_aov)",
    "run_view_aov_device": "the AOV pass is a single-device interface (crt_render_aov_device)",
    "run_view_aov_shading": "the AOV pass is a single-device interface (crt_render_aov_shading)",
    "run_view_aov_shading_device": "the AOV pass is a single-device interface (crt_render_aov_shading_device)",
    "run_view_aov_direct": "the AOV pass is a single-device interface (crt_render_aov_direct)",
    "run_view_aov_direct_device": "the AOV pass is a single-device interface (crt_render_aov_direct_device)",
    "run_view_aov_ao": "the AOV pass is a single-device interface (crt_render_aov_ao)",
    "run_view_aov_ao_device": "the AOV pass is a single-device interface (crt_render_aov_ao_device)",
    "aov_ao_defaults": "the AOV pass is a single-device interface (crt_aov_ao_defaults)",
    "run_view_aov_specular": "the AOV pass is a single-device interface (crt_render_aov_specular)",
    "run_view_aov_specular_device": "the AOV pass is a single-device interface (crt_render_aov_specular_device)",
    "run_view_denoised": "the denoiser is a single-device interface (crt_denoise): gather the frame first",
    "run_view_temporal": "temporal accumulation is a single-device interface (crt_temporal): gather the frame first",
    "run_view_upsampled": "upsampling is a single-device interface (crt_upsample): gather the frames first",
    "intersect": "crt_intersect is a single-device interface",
    "blocked": "crt_intersect is a single-device interface",
    "last_launch_ms": "crt_last_launch_ms is a single-device interface (per-rank kernel times: rank_stats)",
}


def _refusal(name, message):
    def method(self, *a, **k):
        raise NotImplementedError(message)
    method.__name__, method.__qualname__ = name, "MultiRender." + name
    method.__doc__ = "Not on a MultiRender: %s." % message
    return method


for _name, _message in _MULTI_REFUSALS.items():
    setattr(MultiRender, _name, _refusal(_name, _message))


def image_load(path):
    """(x, y, comp, samples (y, x, comp) uint8) of a texture file as the reference's stbi_load(path, &x, &y, &comp, 0) returns them
    (Loader.h:58): PNG, BMP, TGA."""
    x, y, comp = C.c_int32(), C.c_int32(), C.c_int32()
    capi.check(capi.lib().crt_image_load(os.fsencode(path), C.byref(x), C.byref(y), C.byref(comp), None, 0), "crt_image_load")
    a = np.zeros((y.value, x.value, comp.value), dtype=np.uint8)
    capi.check(capi.lib().crt_image_load(os.fsencode(path), C.byref(x), C.byref(y), C.byref(comp), capi.ptr(a), a.size), "crt_image_load")
    return x.value, y.value, comp.value, a


def write_pfm(path, data):
    """Writes a (H, W) or (H, W, 3) float array as a Portable Float Map (crt_write_pfm: "Pf" / "PF", little-endian, rows bottom to
    top in the file; row 0 of `data` is the image top)."""
    a = np.ascontiguousarray(data, dtype=np.float32)
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)):
        raise ValueError("write_pfm needs an (H, W) or (H, W, 3) array, got %r" % (a.shape,))
    ch = 1 if a.ndim == 2 else a.shape[2]
    capi.check(capi.lib().crt_write_pfm(os.fsencode(path), a.shape[1], a.shape[0], ch, capi.ptr(a)), "crt_write_pfm")


def adaptive_defaults():
    """crt_adaptive_defaults as a dict: min_samples, step_samples, threshold, mean_floor."""
    p = capi.AdaptiveParams()
    capi.check(capi.lib().crt_adaptive_defaults(C.byref(p)), "crt_adaptive_defaults")
    return {n: getattr(p, n) for n, _ in p._fields_}


def until_defaults():
    """crt_until_defaults as a dict: min_samples, step_samples, threshold, mean_floor, max_above."""
    p = capi.UntilParams()
    capi.check(capi.lib().crt_until_defaults(C.byref(p)), "crt_until_defaults")
    return {n: getattr(p, n) for n, _ in p._fields_}


def frame_error_defaults():
    """crt_frame_error_defaults as a dict: threshold, mean_floor."""
    thr, floor = _frame_error_settings(None, None)
    return {"threshold": thr, "mean_floor": floor}


def _frame_error_settings(threshold, mean_floor):
    thr, floor = C.c_float(), C.c_float()
    capi.check(capi.lib().crt_frame_error_defaults(C.byref(thr), C.byref(floor)), "crt_frame_error_defaults")
    return (thr.value if threshold is None else float(threshold)), (floor.value if mean_floor is None else float(mean_floor))


def shard_pixels(width, height, rank=0, world=1):
    """The pixels of shard `rank` of `world` of a width x height frame: its 8 x 8 tiles rank, rank + world, ... clipped to the frame."""
    tx, ty = (width + 7) // 8, (height + 7) // 8
    n = 0
    for tile in range(rank, tx * ty, world):
        x, y = tile % tx, tile // tx
        n += min(8, width - 8 * x) * min(8, height - 8 * y)
    return n


class FrameError:
    """crt_frame_error_info (include/crt.h) with what a caller reads from it.  The fields: samples_done, spp, pixels, nan_pixels, above,
    hist (16 bins), sum_variance, sum_mean; threshold and mean_floor are the target's."""

    def __init__(self, fields, threshold, mean_floor):
        self.__dict__.update(fields)
        self.threshold, self.mean_floor = threshold, mean_floor

    def as_dict(self):
        return {k: v for k, v in self.__dict__.items()}

    @property
    def fraction_above(self):
        return self.above / self.pixels if self.pixels else 0.0

    @property
    def rel_rmse(self):
        """The root of the mean variance over the mean of the channel-summed means (plus mean_floor): the frame's relative noise"""
        if not self.pixels:
            return 0.0
        return float(np.sqrt(self.sum_variance / self.pixels) / (self.sum_mean / self.pixels + self.mean_floor))

    def percentile_ratio(self, p):
        """The smallest bin edge 4^k, k in -7 .. 7, such that at least p percent of the pixels have a variance within 4^k times the
        target's (their standard error within 2^k times the threshold's); inf when the last bin or the NaN pixels are needed."""
        need = np.ceil(self.pixels * float(p) / 100.0)
        have = 0
        for b in range(15):
            have += self.hist[b]
            if have >= need:
                return 4.0 ** (b - 7)
        return float("inf")

    def __repr__(self):
        return "FrameError(%s)" % ", ".join("%s=%r" % kv for kv in self.as_dict().items())


def _until_info(info, up):
    d = info.as_dict()
    d["last"] = FrameError(d["last"], float(up.threshold), float(up.mean_floor))
    return d


def _adaptive_params(min_samples=None, step_samples=None, threshold=None, mean_floor=None):
    p = capi.AdaptiveParams()
    capi.check(capi.lib().crt_adaptive_defaults(C.byref(p)), "crt_adaptive_defaults")
    for name, v in (("min_samples", min_samples), ("step_samples", step_samples), ("threshold", threshold), ("mean_floor", mean_floor)):
        if v is not None:
            setattr(p, name, int(v) if name.endswith("samples") else float(v))
    return p


def aov_specular_defaults():
    """crt_aov_specular_defaults as a dict: max_bounces."""
    p = capi.AovSpecularParams()
    capi.check(capi.lib().crt_aov_specular_defaults(C.byref(p)), "crt_aov_specular_defaults")
    return {"max_bounces": int(p.max_bounces)}


def _aov_specular_params(max_bounces=None):
    p = capi.AovSpecularParams()
    capi.check(capi.lib().crt_aov_specular_defaults(C.byref(p)), "crt_aov_specular_defaults")
    if max_bounces is not None:
        p.max_bounces = int(max_bounces)
    return p


def _vp(p):
    return C.c_void_p(p) if p else None


def _defaults(struct, call, width=None, height=None, **settings):
    """A params struct as its defaults call (crt_*_defaults, by name) fills it, then the frame's size if given, then the settings that
    are not None, each as the type of its field."""
    p = struct()
    capi.check(getattr(capi.lib(), call)(C.byref(p)), call)
    if width is not None:
        p.width, p.height = int(width), int(height)
    for name, v in settings.items():
        if v is not None:
            setattr(p, name, type(getattr(p, name))(v))
    return p


def _settings(p, names=None):
    """The settings of a params struct as a dict (names None: every field but the frame's size)."""
    return {n: getattr(p, n) for n in names or [f for f, _ in p._fields_ if f not in ("width", "height")]}


def _image_inputs(who, what, fields, struct=None, needs=None):
    """The host arrays of an image operation.  fields = ((name, array or None, values per pixel), ...): the first is the (H, W, 3) image
    (`what` in the error), the others must be (H, W, 3) or (H, W) with its H and W; needs = (name, what it is) of a buffer that may
    not be None.  Returns them as contiguous float32 arrays (None stays None), and sets the fields of the ctypes `struct` to their
    addresses: the caller keeps the list for as long as the struct is in use."""
    c = np.ascontiguousarray(fields[0][1], dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("%s needs %s, got %r" % (who, what, c.shape))
    if needs is not None and dict((n, a) for n, a, _ in fields)[needs[0]] is None:
        raise ValueError("%s needs %s" % (who, needs[1]))
    h, w = c.shape[:2]
    arrays = [c]
    for name, a, channels in fields[1:]:
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float32)
            shape = (h, w, 3) if channels == 3 else (h, w)
            if a.shape != shape:
                raise ValueError("%s: %s has shape %r, expected %r" % (who, name, a.shape, shape))
        arrays.append(a)
    if struct is not None:
        for (name, _, _), a in zip(fields, arrays):
            if a is not None:
                setattr(struct, name, a.ctypes.data)
    return arrays


def denoise_defaults():
    """crt_denoise_defaults as a dict: iterations and the four sigmas."""
    return _settings(_defaults(capi.DenoiseParams, "crt_denoise_defaults"))


def denoise_var_defaults():
    """crt_denoise_var_defaults as a dict: iterations and the four sigmas of the variance-guided filter."""
    return _settings(_defaults(capi.DenoiseParams, "crt_denoise_var_defaults"))


def _denoise_params(width, height, iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth, var=False):
    return _defaults(capi.DenoiseParams, "crt_denoise_var_defaults" if var else "crt_denoise_defaults", width, height, iterations=iterations,
                     sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_albedo=sigma_albedo, sigma_depth=sigma_depth)


def denoise_scratch_bytes(width, height):
    n = C.c_uint64()
    capi.check(capi.lib().crt_denoise_scratch_bytes(width, height, C.byref(n)), "crt_denoise_scratch_bytes")
    return int(n.value)


def denoise(color, albedo=None, normal=None, depth=None, iterations=None, sigma_color=None, sigma_normal=None, sigma_albedo=None,
            sigma_depth=None, device=0, want_rgb=True, return_info=False):
    """AOV-guided edge-avoiding a-trous filter (crt_denoise, contract: include/crt.h) of an (H, W, 3) float32 image of pre-tone-map
    radiance; albedo, normal (H, W, 3) and depth (H, W) are optional guides, None settings take crt_denoise_defaults.  Returns
    (rgb, mean): the RGB8 tone map (None without want_rgb) and the filtered radiance; with return_info also the crt_denoise_info dict."""
    inputs = capi.DenoiseInputs()
    keep = _image_inputs("denoise", "an (H, W, 3) colour image", (("color", color, 3), ("albedo", albedo, 3), ("normal", normal, 3), ("depth", depth, 1)),
                         inputs)
    h, w = keep[0].shape[:2]
    prm = _denoise_params(w, h, iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth)
    mean = np.zeros((h, w, 3), dtype=np.float32)
    rgb = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb else None
    info = capi.DenoiseInfo()
    capi.check(capi.lib().crt_denoise(device, C.byref(prm), C.byref(inputs), capi.ptr(mean), capi.ptr(rgb), C.byref(info)), "crt_denoise")
    return (rgb, mean, info.as_dict()) if return_info else (rgb, mean)


def denoise_device(width, height, color_ptr, out_mean_ptr, out_rgb_ptr, scratch_ptr, scratch_bytes, albedo_ptr=None, normal_ptr=None,
                   depth_ptr=None, iterations=None, sigma_color=None, sigma_normal=None, sigma_albedo=None, sigma_depth=None, device=0,
                   stream=None, want_info=True):
    """Enqueues the filter with everything in device memory (raw device pointers, crt_denoise_device); the caller owns the scratch
    (denoise_scratch_bytes).  With want_info the call synchronizes the stream and returns the crt_denoise_info dict, else None."""
    inputs = capi.DenoiseInputs(color_ptr or None, albedo_ptr or None, normal_ptr or None, depth_ptr or None)
    prm = _denoise_params(width, height, iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth)
    info = capi.DenoiseInfo()
    capi.check(capi.lib().crt_denoise_device(device, C.byref(prm), C.byref(inputs), _vp(out_mean_ptr), _vp(out_rgb_ptr), _vp(scratch_ptr),
                                             int(scratch_bytes), _vp(stream), C.byref(info) if want_info else None), "crt_denoise_device")
    return info.as_dict() if want_info else None


def _denoise_var_host(who, prm_of, color, variance, albedo, normal, depth, device, want_rgb, want_variance, return_info):
    """denoise_var / denoise_nlm on host arrays: the two calls share their inputs, outputs and info; prm_of(w, h): the params struct"""
    inputs = capi.DenoiseVarInputs()
    keep = _image_inputs(who, "an (H, W, 3) colour image", (("color", color, 3), ("variance", variance, 3), ("albedo", albedo, 3),
                                                            ("normal", normal, 3), ("depth", depth, 1)), inputs,
                         needs=("variance", "the variance buffer (Render.variance)"))
    h, w = keep[0].shape[:2]
    prm = prm_of(w, h)
    mean = np.zeros((h, w, 3), dtype=np.float32)
    rgb = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb else None
    var = np.zeros((h, w), dtype=np.float32) if want_variance else None
    info = capi.DenoiseInfo()
    capi.check(getattr(capi.lib(), "crt_" + who)(device, C.byref(prm), C.byref(inputs), capi.ptr(mean), capi.ptr(rgb), capi.ptr(var), C.byref(info)),
               "crt_" + who)
    out = (rgb, mean, var) if want_variance else (rgb, mean)
    return out + (info.as_dict(),) if return_info else out


def _denoise_var_device(who, prm, color_ptr, variance_ptr, albedo_ptr, normal_ptr, depth_ptr, out_mean_ptr, out_rgb_ptr, out_variance_ptr, scratch_ptr,
                        scratch_bytes, device, stream, want_info):
    """denoise_var_device / denoise_nlm_device: as _denoise_var_host"""
    inputs = capi.DenoiseVarInputs(color_ptr or None, variance_ptr or None, albedo_ptr or None, normal_ptr or None, depth_ptr or None)
    info = capi.DenoiseInfo()
    capi.check(getattr(capi.lib(), who)(device, C.byref(prm), C.byref(inputs), _vp(out_mean_ptr), _vp(out_rgb_ptr), _vp(out_variance_ptr),
                                        _vp(scratch_ptr), int(scratch_bytes), _vp(stream), C.byref(info) if want_info else None), who)
    return info.as_dict() if want_info else None


def denoise_var(color, variance, albedo=None, normal=None, depth=None, iterations=None, sigma_color=None, sigma_normal=None,
                sigma_albedo=None, sigma_depth=None, device=0, want_rgb=True, want_variance=False, return_info=False):
    """Variance-guided form of the filter (crt_denoise_var, contract: include/crt.h): `variance` is the (H, W, 3) buffer of
    Render.variance(); None settings take crt_denoise_var_defaults.  Returns (rgb, mean), with want_variance (rgb, mean, var) -- var
    (H, W) float32, the filter's estimate of the noise left -- and with return_info also the crt_denoise_info dict."""
    return _denoise_var_host("denoise_var", lambda w, h: _denoise_params(w, h, iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth, var=True),
                             color, variance, albedo, normal, depth, device, want_rgb, want_variance, return_info)


def denoise_var_device(width, height, color_ptr, variance_ptr, out_mean_ptr, out_rgb_ptr, out_variance_ptr, scratch_ptr, scratch_bytes,
                       albedo_ptr=None, normal_ptr=None, depth_ptr=None, iterations=None, sigma_color=None, sigma_normal=None,
                       sigma_albedo=None, sigma_depth=None, device=0, stream=None, want_info=True):
    """Enqueues the variance-guided filter with everything in device memory (raw device pointers, crt_denoise_var_device); the scratch
    is that of denoise_device (denoise_scratch_bytes).  With want_info the call synchronizes the stream and returns the info dict."""
    prm = _denoise_params(width, height, iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth, var=True)
    return _denoise_var_device("crt_denoise_var_device", prm, color_ptr, variance_ptr, albedo_ptr, normal_ptr, depth_ptr, out_mean_ptr, out_rgb_ptr,
                               out_variance_ptr, scratch_ptr, scratch_bytes, device, stream, want_info)


_NLM_SETTINGS = ("radius", "patch", "k", "alpha", "sigma_normal", "sigma_albedo", "sigma_depth")


def denoise_nlm_defaults():
    """crt_denoise_nlm_defaults as a dict: radius, patch, k, alpha and the three guide sigmas."""
    return _settings(_defaults(capi.NlmParams, "crt_denoise_nlm_defaults"), _NLM_SETTINGS)


def _nlm_params(width, height, **settings):
    return _defaults(capi.NlmParams, "crt_denoise_nlm_defaults", width, height, **{n: settings.get(n) for n in _NLM_SETTINGS})


def denoise_nlm_scratch_bytes(width, height):
    n = C.c_uint64()
    capi.check(capi.lib().crt_denoise_nlm_scratch_bytes(width, height, C.byref(n)), "crt_denoise_nlm_scratch_bytes")
    return int(n.value)


def denoise_nlm(color, variance, albedo=None, normal=None, depth=None, radius=None, patch=None, k=None, alpha=None, sigma_normal=None,
                sigma_albedo=None, sigma_depth=None, device=0, want_rgb=True, want_variance=False, return_info=False):
    """Non-local means with variance-normalised patch distances, joint with the guides (crt_denoise_nlm, contract: include/crt.h):
    `variance` is the (H, W, 3) buffer of Render.variance(); None settings take crt_denoise_nlm_defaults.  Returns (rgb, mean), with
    want_variance (rgb, mean, var) -- var (H, W) float32 -- and with return_info also the crt_denoise_info dict."""
    settings = dict(radius=radius, patch=patch, k=k, alpha=alpha, sigma_normal=sigma_normal, sigma_albedo=sigma_albedo, sigma_depth=sigma_depth)
    return _denoise_var_host("denoise_nlm", lambda w, h: _nlm_params(w, h, **settings), color, variance, albedo, normal, depth, device, want_rgb,
                             want_variance, return_info)


def denoise_nlm_device(width, height, color_ptr, variance_ptr, out_mean_ptr, out_rgb_ptr, out_variance_ptr, scratch_ptr, scratch_bytes,
                       albedo_ptr=None, normal_ptr=None, depth_ptr=None, radius=None, patch=None, k=None, alpha=None, sigma_normal=None,
                       sigma_albedo=None, sigma_depth=None, device=0, stream=None, want_info=True):
    """Enqueues the non-local-means filter with everything in device memory (raw device pointers, crt_denoise_nlm_device); the caller
    owns the scratch (denoise_nlm_scratch_bytes).  With want_info the call synchronizes the stream and returns the info dict."""
    prm = _nlm_params(width, height, radius=radius, patch=patch, k=k, alpha=alpha, sigma_normal=sigma_normal, sigma_albedo=sigma_albedo,
                      sigma_depth=sigma_depth)
    return _denoise_var_device("crt_denoise_nlm_device", prm, color_ptr, variance_ptr, albedo_ptr, normal_ptr, depth_ptr, out_mean_ptr, out_rgb_ptr,
                               out_variance_ptr, scratch_ptr, scratch_bytes, device, stream, want_info)


_REGRESS_SETTINGS = ("radius", "patch", "k", "alpha", "sigma_normal", "sigma_albedo", "sigma_depth", "sigma_position", "ridge", "features")
_REGRESS_GUIDE_BITS = (("normal", capi.REGRESS_NORMAL), ("albedo", capi.REGRESS_ALBEDO), ("depth", capi.REGRESS_DEPTH))


def denoise_regress_defaults():
    """crt_denoise_regress_defaults as a dict: radius, patch, k, alpha, the four sigmas, ridge and the features mask."""
    return _settings(_defaults(capi.RegressParams, "crt_denoise_regress_defaults"), _REGRESS_SETTINGS)


def _regress_params(who, width, height, settings, given):
    """settings: the caller's, None or absent = crt_denoise_regress_defaults'; given: the guides that are there -- a `features` of None
    is the default mask without the bits of guides that are not given (an explicit mask goes to the library as it is)"""
    unknown = sorted(set(settings) - set(_REGRESS_SETTINGS))
    if unknown:
        raise ValueError("%s: unknown settings %r" % (who, unknown))
    for name in ("radius", "patch", "features"):
        v = settings.get(name)
        if v is not None and (int(v) != v or not 0 <= int(v) < 2 ** 32):
            raise ValueError("%s: %s must be a non-negative integer, got %r" % (who, name, v))
    p = _defaults(capi.RegressParams, "crt_denoise_regress_defaults", width, height, **settings)
    if settings.get("features") is None:
        for name, bit in _REGRESS_GUIDE_BITS:
            if name not in given:
                p.features &= ~bit
    return p


def denoise_regress_scratch_bytes(width, height):
    n = C.c_uint64()
    capi.check(capi.lib().crt_denoise_regress_scratch_bytes(width, height, C.byref(n)), "crt_denoise_regress_scratch_bytes")
    return int(n.value)


def denoise_regress(color, variance, albedo=None, normal=None, depth=None, weight_color=None, weight_variance=None, device=0, want_rgb=True,
                    want_mean=True, return_info=False, **settings):
    """First-order feature regression with non-local-means weights (crt_denoise_regress, contract: include/crt.h): `variance` is the
    (H, W, 3) buffer of Render.variance(); weight_color / weight_variance: the image the weights come from (None: color / variance).
    settings: radius, patch, k, alpha, sigma_normal, sigma_albedo, sigma_depth, sigma_position, ridge, features (REGRESS_* bits); None or
    absent takes crt_denoise_regress_defaults, and a features of None is the default mask less the guides that are not given.  Returns
    (rgb, mean) -- None for the one that is not wanted --, with return_info also the crt_regress_info dict (total_ms, fallback_pixels)."""
    inputs = capi.RegressInputs()
    keep = _image_inputs("denoise_regress", "an (H, W, 3) colour image",
                         (("color", color, 3), ("variance", variance, 3), ("weight_color", weight_color, 3), ("weight_variance", weight_variance, 3),
                          ("albedo", albedo, 3), ("normal", normal, 3), ("depth", depth, 1)), inputs, needs=("variance", "the variance buffer (Render.variance)"))
    h, w = keep[0].shape[:2]
    given = {n for n, a in (("albedo", albedo), ("normal", normal), ("depth", depth)) if a is not None}
    prm = _regress_params("denoise_regress", w, h, settings, given)
    mean = np.zeros((h, w, 3), dtype=np.float32) if want_mean else None
    rgb = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb else None
    info = capi.RegressInfo()
    capi.check(capi.lib().crt_denoise_regress(device, C.byref(prm), C.byref(inputs), capi.ptr(mean), capi.ptr(rgb), C.byref(info)), "crt_denoise_regress")
    return (rgb, mean, info.as_dict()) if return_info else (rgb, mean)


def denoise_regress_device(width, height, color_ptr, variance_ptr, out_mean_ptr, out_rgb_ptr, scratch_ptr, scratch_bytes, albedo_ptr=None,
                           normal_ptr=None, depth_ptr=None, weight_color_ptr=None, weight_variance_ptr=None, device=0, stream=None, want_info=True,
                           **settings):
    """Enqueues the regression filter with everything in device memory (raw device pointers, crt_denoise_regress_device); the caller owns
    the scratch (denoise_regress_scratch_bytes).  settings as denoise_regress.  With want_info the call synchronizes the stream and
    returns the crt_regress_info dict, else None."""
    inputs = capi.RegressInputs(color_ptr or None, variance_ptr or None, weight_color_ptr or None, weight_variance_ptr or None, albedo_ptr or None,
                                normal_ptr or None, depth_ptr or None)
    given = {n for n, a in (("albedo", albedo_ptr), ("normal", normal_ptr), ("depth", depth_ptr)) if a}
    prm = _regress_params("denoise_regress_device", width, height, settings, given)
    info = capi.RegressInfo()
    capi.check(capi.lib().crt_denoise_regress_device(device, C.byref(prm), C.byref(inputs), _vp(out_mean_ptr), _vp(out_rgb_ptr), _vp(scratch_ptr),
                                                     int(scratch_bytes), _vp(stream), C.byref(info) if want_info else None), "crt_denoise_regress_device")
    return info.as_dict() if want_info else None


def modulate_defaults():
    """crt_modulate_defaults as a dict: albedo_floor."""
    return _settings(_defaults(capi.ModulateParams, "crt_modulate_defaults"))


def _modulate_params(width, height, albedo_floor):
    return _defaults(capi.ModulateParams, "crt_modulate_defaults", width, height, albedo_floor=albedo_floor)


def demodulate(color, albedo, emission=None, variance=None, albedo_floor=None, device=0, return_info=False):
    """Radiance to irradiance (crt_demodulate, contract: include/crt.h): (color - emission) / albedo per channel wherever albedo >
    albedo_floor, color - emission elsewhere; all (H, W, 3) float32 -- albedo and emission are diffuse_albedo and emission of
    Render.run_view_aov_shading.  Returns the irradiance, with `variance` (of Render.variance()) the pair (irradiance, variance /
    albedo^2); with return_info also the crt_modulate_info dict."""
    if albedo is None:
        raise ValueError("demodulate needs the albedo buffer (Render.run_view_aov_shading: diffuse_albedo)")
    c, a, e, v = _image_inputs("demodulate", "an (H, W, 3) image", (("color", color, 3), ("albedo", albedo, 3), ("emission", emission, 3),
                                                                    ("variance", variance, 3)))
    h, w = c.shape[:2]
    prm = _modulate_params(w, h, albedo_floor)
    out = np.zeros((h, w, 3), dtype=np.float32)
    ovar = np.zeros((h, w, 3), dtype=np.float32) if v is not None else None
    info = capi.ModulateInfo()
    capi.check(capi.lib().crt_demodulate(device, C.byref(prm), capi.ptr(c), capi.ptr(a), capi.ptr(e), capi.ptr(v), capi.ptr(out), capi.ptr(ovar),
                                         C.byref(info)), "crt_demodulate")
    res = ((out,) if v is None else (out, ovar)) + ((info.as_dict(),) if return_info else ())
    return res[0] if len(res) == 1 else res


def modulate(irradiance, albedo, emission=None, albedo_floor=None, device=0, want_rgb=True, return_info=False):
    """Irradiance back to radiance (crt_modulate): irradiance * albedo wherever albedo > albedo_floor, plus emission.  Returns (rgb,
    mean): the frame's RGB8 tone map (None without want_rgb) and the radiance; with return_info also the crt_modulate_info dict."""
    if albedo is None:
        raise ValueError("modulate needs the albedo buffer (Render.run_view_aov_shading: diffuse_albedo)")
    i, a, e = _image_inputs("modulate", "an (H, W, 3) image", (("irradiance", irradiance, 3), ("albedo", albedo, 3), ("emission", emission, 3)))
    h, w = i.shape[:2]
    prm = _modulate_params(w, h, albedo_floor)
    mean = np.zeros((h, w, 3), dtype=np.float32)
    rgb = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb else None
    info = capi.ModulateInfo()
    capi.check(capi.lib().crt_modulate(device, C.byref(prm), capi.ptr(i), capi.ptr(a), capi.ptr(e), capi.ptr(mean), capi.ptr(rgb), C.byref(info)),
               "crt_modulate")
    return (rgb, mean, info.as_dict()) if return_info else (rgb, mean)


def demodulate_device(width, height, color_ptr, albedo_ptr, out_ptr, emission_ptr=None, variance_ptr=None, out_variance_ptr=None, albedo_floor=None,
                      device=0, stream=None, want_info=True):
    """Enqueues crt_demodulate_device on raw device pointers.  With want_info the call synchronizes the stream and returns the
    crt_modulate_info dict, else None."""
    prm = _modulate_params(width, height, albedo_floor)
    info = capi.ModulateInfo()
    capi.check(capi.lib().crt_demodulate_device(device, C.byref(prm), _vp(color_ptr), _vp(albedo_ptr), _vp(emission_ptr), _vp(variance_ptr), _vp(out_ptr),
                                                _vp(out_variance_ptr), _vp(stream), C.byref(info) if want_info else None), "crt_demodulate_device")
    return info.as_dict() if want_info else None


def modulate_device(width, height, irradiance_ptr, albedo_ptr, out_mean_ptr, out_rgb_ptr=None, emission_ptr=None, albedo_floor=None, device=0,
                    stream=None, want_info=True):
    """Enqueues crt_modulate_device on raw device pointers; out_mean_ptr or out_rgb_ptr may be None, not both.  want_info as
    demodulate_device."""
    prm = _modulate_params(width, height, albedo_floor)
    info = capi.ModulateInfo()
    capi.check(capi.lib().crt_modulate_device(device, C.byref(prm), _vp(irradiance_ptr), _vp(albedo_ptr), _vp(emission_ptr), _vp(out_mean_ptr),
                                              _vp(out_rgb_ptr), _vp(stream), C.byref(info) if want_info else None), "crt_modulate_device")
    return info.as_dict() if want_info else None


_demodulate, _modulate = demodulate, modulate  # (the Render methods have a `demodulate` argument of their own)


_UPSAMPLE_SETTINGS = ("radius", "min_weight", "sigma_normal", "sigma_albedo", "sigma_depth")


def upsample_defaults():
    """crt_upsample_defaults as a dict: radius, min_weight and the three guide sigmas."""
    return _settings(_defaults(capi.UpsampleParams, "crt_upsample_defaults"), _UPSAMPLE_SETTINGS)


def _upsample_params(who, width, height, low_width, low_height, settings):
    unknown = set(settings) - set(_UPSAMPLE_SETTINGS)
    if unknown:
        raise ValueError("%s: unknown settings %r" % (who, sorted(unknown)))
    r = settings.get("radius")
    if r is not None and (int(r) != r or not 0 <= int(r) < 2 ** 32):
        raise ValueError("%s: radius must be an integer 1 .. 4, got %r" % (who, r))
    p = _defaults(capi.UpsampleParams, "crt_upsample_defaults", width, height, **settings)
    p.low_width, p.low_height = int(low_width), int(low_height)
    return p


def upsample(low, width, height, guides=None, device=0, want_rgb=True, return_info=False, **settings):
    """Guide-driven upsampling (crt_upsample, contract: include/crt.h) of a low-resolution image to width x height.  low: dict of the
    (h, w, 3) float32 image `color` and optionally its `variance` (h, w, 3) and the low-resolution guides albedo, normal (h, w, 3) and
    depth (h, w); guides: dict of the same guides at (height, width), or None for the plain tent interpolation.  A guide counts when it
    is given at both sizes.  settings: radius, min_weight, sigma_normal, sigma_albedo, sigma_depth; None or absent takes
    crt_upsample_defaults.  Returns (rgb, color), with a variance (rgb, color, variance): the RGB8 tone map (None without want_rgb), the
    upsampled image and its variance; with return_info also the crt_upsample_info dict (total_ms, fallback_pixels)."""
    for name, d, known in (("low", low, capi.UpsampleLow), ("guides", guides or {}, capi.UpsampleGuides)):
        unknown = set(d) - {n for n, _ in known._fields_}
        if unknown:
            raise ValueError("upsample: unknown %s buffers %r" % (name, sorted(unknown)))
    if low.get("color") is None:
        raise ValueError("upsample needs the low-resolution image (low['color'])")
    lo, hi = capi.UpsampleLow(), capi.UpsampleGuides()
    keep = _image_inputs("upsample", "an (h, w, 3) low-resolution image", (("color", low["color"], 3), ("variance", low.get("variance"), 3),
                                                                           ("albedo", low.get("albedo"), 3), ("normal", low.get("normal"), 3),
                                                                           ("depth", low.get("depth"), 1)), lo)
    lh, lw = keep[0].shape[:2]
    width, height = int(width), int(height)
    if guides is not None:
        for name, channels in (("albedo", 3), ("normal", 3), ("depth", 1)):
            a = guides.get(name)
            if a is None:
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != ((height, width, 3) if channels == 3 else (height, width)):
                raise ValueError("upsample: the %s guide has shape %r for a %d x %d output" % (name, a.shape, width, height))
            keep.append(a)
            setattr(hi, name, a.ctypes.data)
    prm = _upsample_params("upsample", width, height, lw, lh, settings)
    color = np.zeros((height, width, 3), dtype=np.float32)
    var = np.zeros((height, width, 3), dtype=np.float32) if keep[1] is not None else None
    rgb = np.zeros((height, width, 3), dtype=np.uint8) if want_rgb else None
    info = capi.UpsampleInfo()
    capi.check(capi.lib().crt_upsample(device, C.byref(prm), C.byref(lo), C.byref(hi) if guides is not None else None, capi.ptr(color), capi.ptr(var),
                                       capi.ptr(rgb), C.byref(info)), "crt_upsample")
    out = (rgb, color) if var is None else (rgb, color, var)
    return out + (info.as_dict(),) if return_info else out


def upsample_device(width, height, low_width, low_height, low_ptrs, out_color_ptr, out_variance_ptr=None, out_rgb_ptr=None, guide_ptrs=None, device=0,
                    stream=None, want_info=True, **settings):
    """Enqueues crt_upsample_device with everything in device memory: low_ptrs / guide_ptrs = {name: raw device pointer} with the names of
    upsample()'s dicts (guide_ptrs None: no guides).  out_color_ptr or out_rgb_ptr may be None, not both.  With want_info the call
    synchronizes the stream and returns the crt_upsample_info dict, else None."""
    def fill(struct, ptrs):
        for name, p in ptrs.items():
            if name not in {n for n, _ in struct._fields_}:
                raise ValueError("upsample_device: unknown buffer %r" % name)
            setattr(struct, name, int(p) if p else None)
        return struct
    lo = fill(capi.UpsampleLow(), low_ptrs)
    hi = fill(capi.UpsampleGuides(), guide_ptrs) if guide_ptrs is not None else None
    prm = _upsample_params("upsample_device", width, height, low_width, low_height, settings)
    info = capi.UpsampleInfo()
    capi.check(capi.lib().crt_upsample_device(device, C.byref(prm), C.byref(lo), C.byref(hi) if hi is not None else None, _vp(out_color_ptr),
                                              _vp(out_variance_ptr), _vp(out_rgb_ptr), _vp(stream), C.byref(info) if want_info else None),
               "crt_upsample_device")
    return info.as_dict() if want_info else None


_PYRAMID_PLANES = (("color", 3), ("variance", 3), ("albedo", 3), ("normal", 3), ("depth", 1))
MAX_SCALES = 4


def pixel_filter_defaults():
    """crt_pixel_filter_defaults as a dict: kind ("tent") and radius (1)."""
    p = capi.PixelFilter()
    capi.check(capi.lib().crt_pixel_filter_defaults(C.byref(p)), "crt_pixel_filter_defaults")
    return {"kind": {v: k for k, v in capi.PIXEL_FILTER_KINDS.items()}[int(p.kind)], "radius": float(p.radius)}


def _pixel_filter(spec):
    """"box" | "tent" | "mitchell" | dict(kind=, radius=) -> crt_pixel_filter; a kind alone takes the radius the contract ties to it
    (box 0.5: the frame's own filter, tent 1, mitchell 2).  kind may be a name or a CRT_PIXEL_FILTER_* number."""
    if isinstance(spec, str):
        spec = {"kind": spec}
    unknown = set(spec) - {"kind", "radius"}
    if unknown or "kind" not in spec:
        raise ValueError("set_pixel_filter: a filter is a kind name or dict(kind=, radius=), got %r" % (spec,))
    kind = spec["kind"]
    if isinstance(kind, str):
        if kind not in capi.PIXEL_FILTER_KINDS:
            raise ValueError("set_pixel_filter: unknown kind %r (one of %s)" % (kind, ", ".join(capi.PIXEL_FILTER_KINDS)))
        kind = capi.PIXEL_FILTER_KINDS[kind]
    radius = spec.get("radius")
    if radius is None:
        radius = {capi.PIXEL_FILTER_BOX: 0.5, capi.PIXEL_FILTER_TENT: 1.0}.get(int(kind), 2.0)
    return capi.PixelFilter(int(kind), float(radius))


def pyramid_size(width, height):
    """(low_width, low_height) of the next coarser scale: ((width + 1) // 2, (height + 1) // 2) (crt_pyramid_size)."""
    lw, lh = C.c_uint32(), C.c_uint32()
    capi.check(capi.lib().crt_pyramid_size(int(width), int(height), C.byref(lw), C.byref(lh)), "crt_pyramid_size")
    return int(lw.value), int(lh.value)


def _pyramid_params(width, height):
    p = capi.PyramidParams()
    p.width, p.height = int(width), int(height)
    p.low_width, p.low_height = (p.width + 1) // 2, (p.height + 1) // 2
    return p


def pyramid_down(color, variance=None, albedo=None, normal=None, depth=None, device=0, return_info=False):
    """The variance-aware 2 x reduction of a frame and its guides (crt_pyramid_down, contract: include/crt.h): color (H, W, 3) float32;
    variance, albedo, normal (H, W, 3) and depth (H, W) are optional.  Returns a dict of the planes that were given at
    ((H + 1) // 2, (W + 1) // 2); with return_info the pair (dict, crt_pyramid_info dict)."""
    inputs, outputs = capi.PyramidPlanes(), capi.PyramidPlanes()
    keep = _image_inputs("pyramid_down", "an (H, W, 3) colour image", (("color", color, 3), ("variance", variance, 3), ("albedo", albedo, 3),
                                                                      ("normal", normal, 3), ("depth", depth, 1)), inputs)
    h, w = keep[0].shape[:2]
    prm = _pyramid_params(w, h)
    out = {}
    for (name, channels), a in zip(_PYRAMID_PLANES, keep):
        if a is not None:
            out[name] = np.zeros((prm.low_height, prm.low_width, 3) if channels == 3 else (prm.low_height, prm.low_width), dtype=np.float32)
            setattr(outputs, name, out[name].ctypes.data)
    info = capi.PyramidInfo()
    capi.check(capi.lib().crt_pyramid_down(device, C.byref(prm), C.byref(inputs), C.byref(outputs), C.byref(info)), "crt_pyramid_down")
    return (out, info.as_dict()) if return_info else out


def pyramid_down_device(width, height, in_ptrs, out_ptrs, device=0, stream=None, want_info=True):
    """Enqueues crt_pyramid_down_device with everything in device memory: in_ptrs / out_ptrs = {name: raw device pointer} with the names
    color, variance, albedo, normal, depth; the outputs have ((height + 1) // 2) x ((width + 1) // 2) pixels.  With want_info the call
    synchronizes the stream and returns the crt_pyramid_info dict, else None."""
    def fill(ptrs):
        struct = capi.PyramidPlanes()
        for name, p in ptrs.items():
            if name not in dict(_PYRAMID_PLANES):
                raise ValueError("pyramid_down_device: unknown buffer %r" % name)
            setattr(struct, name, int(p) if p else None)
        return struct
    prm = _pyramid_params(width, height)
    info = capi.PyramidInfo()
    capi.check(capi.lib().crt_pyramid_down_device(device, C.byref(prm), C.byref(fill(in_ptrs)), C.byref(fill(out_ptrs)), _vp(stream),
                                                  C.byref(info) if want_info else None), "crt_pyramid_down_device")
    return info.as_dict() if want_info else None


def pyramid_merge(fine, coarse, device=0, want_rgb=True, want_mean=True, return_info=False):
    """The pyramid's merge (crt_pyramid_merge, contract: include/crt.h): `fine` (H, W, 3), the filtered fine scale, with its low
    frequencies replaced by `coarse` ((H + 1) // 2, (W + 1) // 2, 3), the finished result of the coarser scale.  Returns (rgb, mean) --
    None for the one that is not wanted --, with return_info also the crt_pyramid_info dict.  There is no variance of the result."""
    f = np.ascontiguousarray(fine, dtype=np.float32)
    if f.ndim != 3 or f.shape[2] != 3:
        raise ValueError("pyramid_merge needs an (H, W, 3) fine image, got %r" % (f.shape,))
    h, w = f.shape[:2]
    prm = _pyramid_params(w, h)
    c = np.ascontiguousarray(coarse, dtype=np.float32)
    if c.shape != (prm.low_height, prm.low_width, 3):
        raise ValueError("pyramid_merge: the coarse image has shape %r, expected %r" % (c.shape, (prm.low_height, prm.low_width, 3)))
    mean = np.zeros((h, w, 3), dtype=np.float32) if want_mean else None
    rgb = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb else None
    info = capi.PyramidInfo()
    capi.check(capi.lib().crt_pyramid_merge(device, C.byref(prm), capi.ptr(f), capi.ptr(c), capi.ptr(mean), capi.ptr(rgb), C.byref(info)),
               "crt_pyramid_merge")
    return (rgb, mean, info.as_dict()) if return_info else (rgb, mean)


def pyramid_merge_device(width, height, fine_ptr, coarse_ptr, out_color_ptr, out_rgb_ptr=None, device=0, stream=None, want_info=True):
    """Enqueues crt_pyramid_merge_device on raw device pointers; out_color_ptr or out_rgb_ptr may be None, not both.  want_info as
    pyramid_down_device."""
    prm = _pyramid_params(width, height)
    info = capi.PyramidInfo()
    capi.check(capi.lib().crt_pyramid_merge_device(device, C.byref(prm), _vp(fine_ptr), _vp(coarse_ptr), _vp(out_color_ptr), _vp(out_rgb_ptr),
                                                   _vp(stream), C.byref(info) if want_info else None), "crt_pyramid_merge_device")
    return info.as_dict() if want_info else None


def _check_scales(who, scales):
    if isinstance(scales, bool) or int(scales) != scales or not 1 <= int(scales) <= MAX_SCALES:
        raise ValueError("%s: scales must be an integer 1 .. %d, got %r" % (who, MAX_SCALES, scales))
    return int(scales)


_ATROUS_SETTINGS = ("iterations", "sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth")
# the single-frame filters: name: (the host call, the settings it accepts, whether it takes a variance, whether it can take its weights from
# another image)
_FILTERS = {"atrous": (denoise, _ATROUS_SETTINGS, False, False), "var": (denoise_var, _ATROUS_SETTINGS, True, False),
            "nlm": (denoise_nlm, _NLM_SETTINGS, True, False), "reg": (denoise_regress, _REGRESS_SETTINGS, True, True)}


def _run_filter(name, color, variance, guides, settings, device, want_rgb, weights=None):
    """Filter `name` of _FILTERS on a frame: returns (rgb, mean, info), rgb None without want_rgb.  guides: albedo, normal, depth as
    keywords; settings: the filter's own (None or absent: its default); weights: the image a filter that can takes its weights from,
    with `variance` as that image's variance.  The one place that knows how the calls' argument lists differ."""
    call, _, takes_variance, takes_weights = _FILTERS[name]
    if takes_weights and weights is not None:
        settings = dict(settings, weight_color=weights, weight_variance=variance)
    return call(*((color, variance) if takes_variance else (color,)), device=device, want_rgb=want_rgb, return_info=True, **guides, **settings)


def _select_request(who, candidates):
    """the candidate names of a run_view_selected form, checked"""
    names = tuple(candidates)
    unknown = [n for n in names if n not in _SELECT_CANDIDATES]
    if unknown or not 1 <= len(names) <= capi.SELECT_MAX_CANDIDATES:
        raise ValueError("%s: candidates must be 1 .. %d of %r, got %r" % (who, capi.SELECT_MAX_CANDIDATES, _SELECT_CANDIDATES, names))
    return names


def _denoise_request(who, variance_guided, iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth, nlm, regress, scales, demodulate):
    """(filter name of _FILTERS, its settings, scales) of the filter arguments of a run_view_denoised form, checked"""
    scales = 1 if scales is None else _check_scales(who, scales)
    name, settings = _legacy_filter(who, variance_guided, iterations, sigma_color,
                                    dict(sigma_normal=sigma_normal, sigma_albedo=sigma_albedo, sigma_depth=sigma_depth), nlm, regress, scales, demodulate)
    return name, settings, scales


def _legacy_filter(who, variance_guided, iterations, sigma_color, sigmas, nlm, regress, scales, demodulate):
    """run_view_denoised's way of choosing a filter as (name, settings) of _FILTERS.  nlm, regress: None or False = not chosen, True =
    its defaults, or a dict of its settings; sigmas: the three guide sigmas, which go to whichever filter is chosen."""
    own = [(key, arg, given, excludes) for key, arg, given, excludes in
           (("nlm", "nlm", nlm, "variance_guided, iterations and sigma_color (the a-trous filter's)"),
            ("reg", "regress", regress, "nlm, variance_guided, iterations and sigma_color")) if given is not None and given is not False]
    if scales > 1 and not (variance_guided or own):
        raise ValueError("%s: scales needs variance_guided, nlm or regress (the pyramid reduces the variance with the frame)" % who)
    name, settings = "var" if variance_guided else "atrous", dict(sigmas, iterations=iterations, sigma_color=sigma_color)
    for key, arg, given, excludes in own:
        if name != "atrous" or iterations is not None or sigma_color is not None:
            raise ValueError("%s: %s excludes %s" % (who, arg, excludes))
        name, settings = key, {} if given is True else dict(given)
        unknown = sorted(set(settings) - set(_FILTERS[key][1]))
        if unknown:
            raise ValueError("%s: unknown %s settings %r" % (who, arg, unknown))
        settings.update({k: v for k, v in sigmas.items() if v is not None})
    if name == "reg" and demodulate:  # irradiance does not follow the albedo: the feature goes, from an explicit mask too
        mask = settings.get("features")
        settings["features"] = (denoise_regress_defaults()["features"] if mask is None else int(mask)) & ~capi.REGRESS_ALBEDO
    return name, settings


def denoise_multiscale(color, variance, albedo=None, normal=None, depth=None, filter="var", scales=2, device=0, want_rgb=True, return_info=False,
                       **settings):
    """A Laplacian pyramid over one of the single-scale filters: the frame and its guides are reduced scales - 1 times (pyramid_down), the
    filter `filter` -- "var" (denoise_var), "nlm" (denoise_nlm) or "reg" (denoise_regress) -- runs with the same `settings` at every
    scale, and the results are merged from the coarsest scale up (pyramid_merge).  scales is 1 .. 4; scales=1 is the filter's own call.
    Returns (rgb, mean); with return_info also a dict: total_ms (the sum of the calls' timers) and calls (a list of (name, width,
    height, total_ms))."""
    who = "denoise_multiscale"
    names = sorted(n for n in _FILTERS if _FILTERS[n][2])  # (the pyramid reduces the variance with the frame)
    if filter not in names:
        raise ValueError("%s: filter must be one of %r, got %r" % (who, names, filter))
    scales = _check_scales(who, scales)
    log = []
    level = {"color": color, "variance": variance, "albedo": albedo, "normal": normal, "depth": depth}
    if variance is None:
        raise ValueError("%s needs the variance buffer (Render.variance)" % who)
    levels = [level]
    for _ in range(scales - 1):
        h, w = np.shape(levels[-1]["color"])[:2]
        low, info = pyramid_down(device=device, return_info=True, **levels[-1])
        log.append(("pyramid_down", w, h, info["total_ms"]))
        levels.append({name: low.get(name) for name, _ in _PYRAMID_PLANES})
    result = None
    for k in range(scales - 1, -1, -1):
        lv = levels[k]
        h, w = np.shape(lv["color"])[:2]
        last = k == 0
        rgb, mean, info = _run_filter(filter, lv["color"], lv["variance"], {g: lv[g] for g in ("albedo", "normal", "depth")}, settings, device,
                                      want_rgb and last and result is None)
        log.append(("denoise_" + filter, w, h, info["total_ms"]))
        if result is not None:
            rgb, mean, info = pyramid_merge(mean, result, device=device, want_rgb=want_rgb and last, return_info=True)
            log.append(("pyramid_merge", w, h, info["total_ms"]))
        result = mean
    out = (rgb, result)
    return out + ({"total_ms": float(sum(c[3] for c in log)), "calls": log},) if return_info else out


_SELECT_SETTINGS = ("error_radius", "blend_radius")
_SELECT_CANDIDATES = ("none", "atrous", "var", "nlm", "reg")


def _select_candidate(name, half, half_variance, guides, device, other=None):
    """Candidate filter `name` of run_view_selected applied to one half frame, with its own defaults; other: the other half frame, where
    "reg" takes its weights"""
    return half if name == "none" else _run_filter(name, half, half_variance, guides, {}, device, False, weights=other)[1]


def filter_select_defaults():
    """crt_filter_select_defaults as a dict: error_radius and blend_radius."""
    return _settings(_defaults(capi.FilterSelectParams, "crt_filter_select_defaults"), _SELECT_SETTINGS)


def filter_select_scratch_bytes(width, height):
    n = C.c_uint64()
    capi.check(capi.lib().crt_filter_select_scratch_bytes(width, height, C.byref(n)), "crt_filter_select_scratch_bytes")
    return int(n.value)


def _select_params(who, width, height, n_candidates, error_radius, blend_radius):
    for name, v in (("error_radius", error_radius), ("blend_radius", blend_radius)):
        if v is not None and (int(v) != v or not 0 <= int(v) < 2 ** 32):
            raise ValueError("%s: %s must be a non-negative integer, got %r" % (who, name, v))
    if not 1 <= n_candidates <= capi.SELECT_MAX_CANDIDATES:
        raise ValueError("%s needs 1 .. %d candidates, got %d" % (who, capi.SELECT_MAX_CANDIDATES, n_candidates))
    return _defaults(capi.FilterSelectParams, "crt_filter_select_defaults", width, height, n_candidates=n_candidates, error_radius=error_radius,
                     blend_radius=blend_radius)


def filter_select(half_a, half_b, half_variance, filtered_a, filtered_b, error_radius=None, blend_radius=None, device=0, want_rgb=True, want_mean=True,
                  want_choice=True, want_error=True, return_info=False):
    """Error-estimated filter selection (crt_filter_select, contract: include/crt.h).  half_a, half_b: the two half frames
    (Render.half_buffers), half_variance: the variance of ONE half's mean (2 x Render.variance), filtered_a / filtered_b: sequences of
    1 .. 4 images, filter k applied to half_a and to half_b; all (H, W, 3) float32.  None radii take crt_filter_select_defaults.
    Returns (rgb, mean, choice, error): the RGB8 tone map, the blended frame, the chosen candidate per pixel (H, W) uint8 and its
    estimated squared error (H, W) float32 -- None for an output that is not wanted; with return_info also the crt_filter_select_info
    dict (total_ms, chosen: pixels per candidate)."""
    fa, fb = list(filtered_a), list(filtered_b)
    if len(fa) != len(fb):
        raise ValueError("filter_select: %d images filtered from half_a, %d from half_b" % (len(fa), len(fb)))
    fields = (("half_a", half_a, 3), ("half_b", half_b, 3), ("half_variance", half_variance, 3)) + \
        tuple(("filtered_a[%d]" % k, x, 3) for k, x in enumerate(fa)) + tuple(("filtered_b[%d]" % k, x, 3) for k, x in enumerate(fb))
    if any(x is None for _, x, _ in fields):
        raise ValueError("filter_select: every input image is required")
    keep = _image_inputs("filter_select", "an (H, W, 3) half frame", fields)
    h, w = keep[0].shape[:2]
    prm = _select_params("filter_select", w, h, len(fa), error_radius, blend_radius)
    inputs = capi.FilterSelectInputs()
    inputs.half_a, inputs.half_b, inputs.half_variance = (x.ctypes.data for x in keep[:3])
    for k in range(len(fa)):
        inputs.filtered_a[k], inputs.filtered_b[k] = keep[3 + k].ctypes.data, keep[3 + len(fa) + k].ctypes.data
    mean = np.zeros((h, w, 3), dtype=np.float32) if want_mean else None
    rgb = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb else None
    choice = np.zeros((h, w), dtype=np.uint8) if want_choice else None
    error = np.zeros((h, w), dtype=np.float32) if want_error else None
    info = capi.FilterSelectInfo()
    capi.check(capi.lib().crt_filter_select(device, C.byref(prm), C.byref(inputs), capi.ptr(mean), capi.ptr(rgb), capi.ptr(choice), capi.ptr(error),
                                            C.byref(info)), "crt_filter_select")
    out = (rgb, mean, choice, error)
    return out + (info.as_dict(),) if return_info else out


def filter_select_device(width, height, half_a_ptr, half_b_ptr, half_variance_ptr, filtered_a_ptrs, filtered_b_ptrs, out_mean_ptr, out_rgb_ptr,
                         scratch_ptr, scratch_bytes, out_choice_ptr=None, out_error_ptr=None, error_radius=None, blend_radius=None, device=0,
                         stream=None, want_info=True):
    """Enqueues crt_filter_select_device with everything in device memory (raw device pointers; filtered_a_ptrs / filtered_b_ptrs:
    sequences of 1 .. 4); the caller owns the scratch (filter_select_scratch_bytes).  out_mean_ptr or out_rgb_ptr may be None, not
    both.  With want_info the call synchronizes the stream and returns the crt_filter_select_info dict, else None."""
    fa, fb = list(filtered_a_ptrs), list(filtered_b_ptrs)
    if len(fa) != len(fb):
        raise ValueError("filter_select_device: %d images filtered from half_a, %d from half_b" % (len(fa), len(fb)))
    prm = _select_params("filter_select_device", width, height, len(fa), error_radius, blend_radius)
    inputs = capi.FilterSelectInputs(half_a_ptr or None, half_b_ptr or None, half_variance_ptr or None)
    for k in range(len(fa)):
        inputs.filtered_a[k], inputs.filtered_b[k] = fa[k] or None, fb[k] or None
    info = capi.FilterSelectInfo()
    capi.check(capi.lib().crt_filter_select_device(device, C.byref(prm), C.byref(inputs), _vp(out_mean_ptr), _vp(out_rgb_ptr), _vp(out_choice_ptr),
                                                   _vp(out_error_ptr), _vp(scratch_ptr), int(scratch_bytes), _vp(stream),
                                                   C.byref(info) if want_info else None), "crt_filter_select_device")
    return info.as_dict() if want_info else None


def _camera(eye_pos, inv_view_mat, fovY):
    cam = capi.Camera()
    cam.eye[:] = [float(v) for v in np.asarray(eye_pos, dtype=np.float32)]
    cam.inv_view[:] = [float(v) for v in np.asarray(inv_view_mat, dtype=np.float32).reshape(9)]
    cam.fov_y = float(np.float32(fovY))
    return cam


def temporal_defaults():
    """crt_temporal_defaults as a dict: depth_tolerance, normal_tolerance, alpha_min."""
    return _settings(_defaults(capi.TemporalParams, "crt_temporal_defaults"), ("depth_tolerance", "normal_tolerance", "alpha_min"))


def temporal_clamp_defaults():
    """crt_temporal_clamp_defaults as a dict: radius, gamma."""
    return _settings(_defaults(capi.TemporalClamp, "crt_temporal_clamp_defaults"))


def _temporal_clamp(clamp):
    """clamp=True (the defaults) or a dict of radius / gamma -> crt_temporal_clamp"""
    c = _defaults(capi.TemporalClamp, "crt_temporal_clamp_defaults")
    if clamp is True:
        return c
    if not isinstance(clamp, dict) or set(clamp) - {"radius", "gamma"}:
        raise ValueError("temporal: clamp must be None, True or a dict of radius / gamma, got %r" % (clamp,))
    if clamp.get("radius") is not None:
        r = int(clamp["radius"])
        if r != clamp["radius"] or not 0 <= r < 2 ** 32:
            raise ValueError("temporal: the clamp's radius must be an integer 1 .. 3, got %r" % (clamp["radius"],))
        c.radius = r
    if clamp.get("gamma") is not None:
        c.gamma = float(clamp["gamma"])
    return c


def temporal_dual_defaults():
    """crt_temporal_dual_defaults as a dict: radius, min_bounces."""
    return _settings(_defaults(capi.TemporalDual, "crt_temporal_dual_defaults"))


_SPECULAR_PLANES = ("path_depth", "bounces", "last_normal")


def _temporal_dual(dual):
    """dual=True (the defaults) or a dict of radius / min_bounces -> crt_temporal_dual"""
    d = _defaults(capi.TemporalDual, "crt_temporal_dual_defaults")
    if dual is True:
        return d
    if not isinstance(dual, dict) or set(dual) - {"radius", "min_bounces"}:
        raise ValueError("temporal: dual must be None, True or a dict of radius / min_bounces, got %r" % (dual,))
    if dual.get("radius") is not None:
        r = int(dual["radius"])
        if r != dual["radius"] or not 0 <= r < 2 ** 32:
            raise ValueError("temporal: the dual reprojection's radius must be an integer 1 .. 3, got %r" % (dual["radius"],))
        d.radius = r
    if dual.get("min_bounces") is not None:
        d.min_bounces = float(dual["min_bounces"])
    return d


def _split_specular(buffers):
    """a frame's dict -> (the dict without the specular planes, the specular planes)"""
    if buffers is None:
        return None, None
    return ({k: v for k, v in buffers.items() if k not in _SPECULAR_PLANES}, {k: v for k, v in buffers.items() if k in _SPECULAR_PLANES})


def _specular_struct(planes, h, w, keep):
    """the specular planes of a frame's dict (host arrays) -> crt_temporal_specular_planes"""
    s = capi.TemporalSpecularPlanes()
    for name in _SPECULAR_PLANES:
        a = planes.get(name)
        if a is None:
            continue
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape != ((h, w, 3) if name == "last_normal" else (h, w)):
            raise ValueError("temporal: %s has shape %r for a %d x %d frame" % (name, a.shape, w, h))
        keep.append(a)
        setattr(s, name, a.ctypes.data)
    return s


def _temporal_params(width, height, camera, prev_camera, depth_tolerance, normal_tolerance, alpha_min):
    p = _defaults(capi.TemporalParams, "crt_temporal_defaults", width, height, depth_tolerance=depth_tolerance, normal_tolerance=normal_tolerance,
                  alpha_min=alpha_min)
    p.cur = _camera(*camera)
    p.prev = _camera(*(prev_camera if prev_camera is not None else camera))
    return p


# the buffers of crt_temporal_frame / crt_temporal_history: name -> (values per pixel, numpy type)
_TEMPORAL_BUFFERS = {"color": (3, np.float32), "variance": (3, np.float32), "history": (1, np.float32), "depth": (1, np.float32),
                     "normal": (3, np.float32), "id": (1, np.int32)}


def _temporal_struct(struct, buffers, h, w, keep):
    for name, _ in struct._fields_:
        a = buffers.get(name)
        if a is None:
            continue
        ch, dt = _TEMPORAL_BUFFERS[name]
        a = np.ascontiguousarray(a, dtype=dt)
        if a.shape != ((h, w, 3) if ch == 3 else (h, w)):
            raise ValueError("temporal: %s has shape %r for a %d x %d frame" % (name, a.shape, w, h))
        keep.append(a)
        setattr(struct, name, a.ctypes.data)
    unknown = set(buffers) - {n for n, _ in struct._fields_}
    if unknown:
        raise ValueError("temporal: unknown buffers %r" % sorted(unknown))
    return struct


def _moment_planes(moments, h, w, keep):
    """moments=dict(m1=, m2=) of the history -> crt_temporal_moment_planes"""
    if not isinstance(moments, dict) or set(moments) != {"m1", "m2"}:
        raise ValueError("temporal: moments must be None, True or a dict of m1 and m2, got %r" % (moments,))
    planes = capi.TemporalMomentPlanes()
    for name in ("m1", "m2"):
        a = np.ascontiguousarray(moments[name], dtype=np.float32)
        if a.shape != (h, w, 3):
            raise ValueError("temporal: %s has shape %r for a %d x %d frame" % (name, a.shape, w, h))
        keep.append(a)
        setattr(planes, name, a.ctypes.data)
    return planes


def temporal(cur, camera, prev=None, prev_camera=None, depth_tolerance=None, normal_tolerance=None, alpha_min=None, device=0, want_rgb=True,
             return_info=False, clamp=None, moments=None, dual=None):
    """Temporal accumulation with reprojection (crt_temporal, contract: include/crt.h).  cur: dict of the current frame -- color
    (H, W, 3), depth (H, W), optionally variance, normal (H, W, 3) and id (H, W) int32; prev: dict of the history -- color, history,
    depth, and variance / normal / id as cur has them -- or None for a first frame; camera, prev_camera: (eye, inv_view, fov_y) of the
    two frames.  None settings take crt_temporal_defaults.  Returns (rgb, color, variance, history): the tone map (None without
    want_rgb), the accumulated colour, its variance (None if cur has none) and the frames accumulated per pixel; with return_info
    also the crt_temporal_info dict.  clamp: None (crt_temporal), True or a dict of radius / gamma (crt_temporal_clamped with its defaults /
    with these values: the history is clamped to its neighbourhood in the current frame, and the info dict gains `clamped`).
    moments: None, or -- crt_temporal_moments -- the dict(m1=, m2=) of the history's moment planes (True for a first frame, where there is
    no history): the call then returns (rgb, color, variance, history, m1, m2), the info dict has `clamped` (0 without a clamp), and
    m1 / m2 / history are what variance_estimate takes.
    dual: None, or -- crt_temporal_dual -- True or a dict of radius / min_bounces: cur and prev then also hold path_depth and bounces
    (H, W) and optionally last_normal (H, W, 3) as Render.run_view_aov_specular returns them, a mirror pixel also tries the history its
    virtual image points at, and the info dict gains `clamped` (0 without a clamp), `virtual_tried` and `virtual_taken`.  Not with
    moments (ValueError)."""
    if dual is not None and moments is not None:
        raise ValueError("temporal: dual and moments cannot be combined (crt_temporal_moments has no dual form)")
    if dual is not None:
        dual = _temporal_dual(dual)
        cur, cur_spec = _split_specular(cur)
        prev, prev_spec = _split_specular(prev)
    c = np.ascontiguousarray(cur["color"], dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("temporal needs an (H, W, 3) colour image, got %r" % (c.shape,))
    if prev is not None and prev_camera is None:
        raise ValueError("temporal: a history needs the camera it was made with")
    h, w = c.shape[:2]
    keep = []
    fc = _temporal_struct(capi.TemporalFrame(), cur, h, w, keep)
    fp = _temporal_struct(capi.TemporalHistory(), prev, h, w, keep) if prev is not None else None
    prm = _temporal_params(w, h, camera, prev_camera, depth_tolerance, normal_tolerance, alpha_min)
    color = np.zeros((h, w, 3), dtype=np.float32)
    var = np.zeros((h, w, 3), dtype=np.float32) if cur.get("variance") is not None else None
    hist = np.zeros((h, w), dtype=np.float32)
    rgb = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb else None
    if moments is not None:
        if (moments is True) != (prev is None):
            raise ValueError("temporal: moments=True goes with a first frame, a dict of m1 and m2 with a history")
        planes = _moment_planes(moments, h, w, keep) if prev is not None else None
        m1, m2 = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w, 3), dtype=np.float32)
        info = capi.TemporalClampInfo()
        capi.check(capi.lib().crt_temporal_moments(device, C.byref(prm), C.byref(_temporal_clamp(clamp)) if clamp is not None else None, C.byref(fc),
                                                   C.byref(fp) if fp is not None else None, C.byref(planes) if planes is not None else None,
                                                   capi.ptr(color), capi.ptr(var), capi.ptr(hist), capi.ptr(m1), capi.ptr(m2), capi.ptr(rgb),
                                                   C.byref(info)), "crt_temporal_moments")
        out = (rgb, color, var, hist, m1, m2)
        return out + (info.as_dict(),) if return_info else out
    if dual is not None:
        sc = _specular_struct(cur_spec, h, w, keep)
        sp = _specular_struct(prev_spec, h, w, keep) if prev is not None else None
        info = capi.TemporalDualInfo()
        capi.check(capi.lib().crt_temporal_dual(device, C.byref(prm), C.byref(_temporal_clamp(clamp)) if clamp is not None else None, C.byref(dual),
                                                C.byref(fc), C.byref(sc), C.byref(fp) if fp is not None else None,
                                                C.byref(sp) if sp is not None else None, capi.ptr(color), capi.ptr(var), capi.ptr(hist), capi.ptr(rgb),
                                                C.byref(info)), "crt_temporal_dual")
    elif clamp is None:
        info = capi.TemporalInfo()
        capi.check(capi.lib().crt_temporal(device, C.byref(prm), C.byref(fc), C.byref(fp) if fp is not None else None, capi.ptr(color), capi.ptr(var),
                                           capi.ptr(hist), capi.ptr(rgb), C.byref(info)), "crt_temporal")
    else:
        info = capi.TemporalClampInfo()
        capi.check(capi.lib().crt_temporal_clamped(device, C.byref(prm), C.byref(_temporal_clamp(clamp)), C.byref(fc), C.byref(fp) if fp is not None else None,
                                                   capi.ptr(color), capi.ptr(var), capi.ptr(hist), capi.ptr(rgb), C.byref(info)), "crt_temporal_clamped")
    out = (rgb, color, var, hist)
    return out + (info.as_dict(),) if return_info else out


def temporal_device(width, height, camera, cur_ptrs, out_color_ptr, out_history_ptr, out_variance_ptr=None, out_rgb_ptr=None, prev_ptrs=None,
                    prev_camera=None, depth_tolerance=None, normal_tolerance=None, alpha_min=None, device=0, stream=None, want_info=True, clamp=None,
                    moments=None, dual=None):
    """Enqueues crt_temporal_device with everything in device memory: cur_ptrs / prev_ptrs = {name: raw device pointer} with the names of
    temporal()'s dicts (prev_ptrs None: no history).  With want_info the call synchronizes the stream and returns the crt_temporal_info
    dict, else None.  clamp: as temporal() (crt_temporal_clamped_device; the dict gains `clamped`).  moments: None, or
    dict(out_m1=, out_m2=) of raw device pointers and, with a history, m1= and m2= of its planes (crt_temporal_moments_device).
    dual: as temporal() (crt_temporal_dual_device): cur_ptrs / prev_ptrs then also hold path_depth, bounces and optionally last_normal."""
    if dual is not None and moments is not None:
        raise ValueError("temporal_device: dual and moments cannot be combined (crt_temporal_moments has no dual form)")
    if dual is not None:
        dual = _temporal_dual(dual)
        cur_ptrs, cur_spec = _split_specular(cur_ptrs)
        prev_ptrs, prev_spec = _split_specular(prev_ptrs)

    def fill(struct, ptrs):
        for name, p in ptrs.items():
            if name not in {n for n, _ in struct._fields_}:
                raise ValueError("temporal_device: unknown buffer %r" % name)
            setattr(struct, name, int(p) if p else None)
        return struct
    fc = fill(capi.TemporalFrame(), cur_ptrs)
    fp = fill(capi.TemporalHistory(), prev_ptrs) if prev_ptrs is not None else None
    prm = _temporal_params(width, height, camera, prev_camera, depth_tolerance, normal_tolerance, alpha_min)
    if moments is not None:
        if not isinstance(moments, dict) or set(moments) - {"m1", "m2", "out_m1", "out_m2"}:
            raise ValueError("temporal_device: moments must be None or a dict of out_m1, out_m2 and the history's m1, m2, got %r" % (moments,))
        planes = None
        if moments.get("m1") or moments.get("m2"):
            planes = capi.TemporalMomentPlanes(moments.get("m1") or None, moments.get("m2") or None)
        info = capi.TemporalClampInfo()
        capi.check(capi.lib().crt_temporal_moments_device(device, C.byref(prm), C.byref(_temporal_clamp(clamp)) if clamp is not None else None, C.byref(fc),
                                                          C.byref(fp) if fp is not None else None, C.byref(planes) if planes is not None else None,
                                                          _vp(out_color_ptr), _vp(out_variance_ptr), _vp(out_history_ptr), _vp(moments.get("out_m1")),
                                                          _vp(moments.get("out_m2")), _vp(out_rgb_ptr), _vp(stream), C.byref(info) if want_info else None),
                   "crt_temporal_moments_device")
        return info.as_dict() if want_info else None
    if dual is not None:
        sc = capi.TemporalSpecularPlanes(**{k: int(v) if v else None for k, v in cur_spec.items()})
        sp = capi.TemporalSpecularPlanes(**{k: int(v) if v else None for k, v in prev_spec.items()}) if prev_ptrs is not None else None
        info = capi.TemporalDualInfo()
        capi.check(capi.lib().crt_temporal_dual_device(device, C.byref(prm), C.byref(_temporal_clamp(clamp)) if clamp is not None else None,
                                                       C.byref(dual), C.byref(fc), C.byref(sc), C.byref(fp) if fp is not None else None,
                                                       C.byref(sp) if sp is not None else None, _vp(out_color_ptr), _vp(out_variance_ptr),
                                                       _vp(out_history_ptr), _vp(out_rgb_ptr), _vp(stream), C.byref(info) if want_info else None),
                   "crt_temporal_dual_device")
    elif clamp is None:
        info = capi.TemporalInfo()
        capi.check(capi.lib().crt_temporal_device(device, C.byref(prm), C.byref(fc), C.byref(fp) if fp is not None else None, _vp(out_color_ptr),
                                                  _vp(out_variance_ptr), _vp(out_history_ptr), _vp(out_rgb_ptr), _vp(stream),
                                                  C.byref(info) if want_info else None), "crt_temporal_device")
    else:
        info = capi.TemporalClampInfo()
        capi.check(capi.lib().crt_temporal_clamped_device(device, C.byref(prm), C.byref(_temporal_clamp(clamp)), C.byref(fc),
                                                          C.byref(fp) if fp is not None else None, _vp(out_color_ptr), _vp(out_variance_ptr),
                                                          _vp(out_history_ptr), _vp(out_rgb_ptr), _vp(stream), C.byref(info) if want_info else None),
                   "crt_temporal_clamped_device")
    return info.as_dict() if want_info else None


_ESTIMATE_SETTINGS = ("min_history", "radius", "sigma_normal", "sigma_depth", "of_mean", "history_cap")
# What this module and crt_cli choose where the library's default (of_mean 0, SVGF's) is not asked for by name: the variance of the
# accumulated mean, which is what the filter is handed (docs/experiments.md, "Variance from temporal moments")
ESTIMATE_OF_MEAN = 1


def variance_estimate_defaults():
    """crt_variance_estimate_defaults as a dict: min_history, radius, sigma_normal, sigma_depth, of_mean, history_cap -- the library's."""
    return _settings(_defaults(capi.VarianceEstimateParams, "crt_variance_estimate_defaults"), _ESTIMATE_SETTINGS)


def _estimate_params(width, height, settings):
    unknown = set(settings) - set(_ESTIMATE_SETTINGS)
    if unknown:
        raise ValueError("variance_estimate: unknown settings %r" % sorted(unknown))
    p = _defaults(capi.VarianceEstimateParams, "crt_variance_estimate_defaults", width, height, of_mean=ESTIMATE_OF_MEAN)
    for name, v in settings.items():
        if v is None:
            continue
        if name in ("min_history", "radius", "of_mean"):
            if int(v) != v or not 0 <= int(v) < 2 ** 32:
                raise ValueError("variance_estimate: %s must be a non-negative integer, got %r" % (name, v))
            v = int(v)
        setattr(p, name, v)
    return p


def variance_estimate(m1, m2, history, normal=None, depth=None, device=0, return_info=False, **settings):
    """Per-pixel variance from temporal moments (crt_variance_estimate, contract: include/crt.h): m1, m2 (H, W, 3) and history (H, W) as
    temporal(moments=...) returns them, normal / depth the current frame's AOVs (optional).  settings: min_history, radius, sigma_normal,
    sigma_depth, of_mean, history_cap; None or absent takes crt_variance_estimate_defaults, except of_mean, which is 1 here (the variance
    of the accumulated mean: docs/experiments.md).  Returns the (H, W, 3) variance, what denoise_var takes; with return_info also the
    crt_variance_estimate_info dict (total_ms, spatial)."""
    inputs = capi.VarianceEstimateInputs()
    keep = _image_inputs("variance_estimate", "(H, W, 3) moments", (("m1", m1, 3), ("m2", m2, 3), ("history", history, 1), ("normal", normal, 3),
                                                                    ("depth", depth, 1)), inputs)
    h, w = keep[0].shape[:2]
    prm = _estimate_params(w, h, settings)
    out = np.zeros((h, w, 3), dtype=np.float32)
    info = capi.VarianceEstimateInfo()
    capi.check(capi.lib().crt_variance_estimate(device, C.byref(prm), C.byref(inputs), capi.ptr(out), C.byref(info)), "crt_variance_estimate")
    return (out, info.as_dict()) if return_info else out


def variance_estimate_device(width, height, m1_ptr, m2_ptr, history_ptr, out_variance_ptr, normal_ptr=None, depth_ptr=None, device=0, stream=None,
                             want_info=True, **settings):
    """Enqueues crt_variance_estimate_device with everything in device memory (raw device pointers); settings as variance_estimate.  With
    want_info the call synchronizes the stream and returns the info dict, else None."""
    inputs = capi.VarianceEstimateInputs(m1_ptr or None, m2_ptr or None, history_ptr or None, normal_ptr or None, depth_ptr or None)
    prm = _estimate_params(width, height, settings)
    info = capi.VarianceEstimateInfo()
    capi.check(capi.lib().crt_variance_estimate_device(device, C.byref(prm), C.byref(inputs), _vp(out_variance_ptr), _vp(stream),
                                                       C.byref(info) if want_info else None), "crt_variance_estimate_device")
    return info.as_dict() if want_info else None


def shard_slots(width, height, rank, world):
    n = C.c_uint64()
    capi.check(capi.lib().crt_shard_slots(width, height, rank, world, C.byref(n)), "crt_shard_slots")
    return int(n.value)


def device_count():
    n = C.c_int()
    capi.check(capi.lib().crt_device_count(C.byref(n)), "crt_device_count")
    return n.value


def device_math(fn, a, b=None, device=0):
    a = np.ascontiguousarray(a, dtype=np.float32)
    bb = np.ascontiguousarray(b, dtype=np.float32) if b is not None else None
    out = np.zeros_like(a)
    capi.check(capi.lib().crt_device_math(device, fn.encode(), a.size, capi.ptr(a), capi.ptr(bb), capi.ptr(out)),
               "crt_device_math")
    return out


def device_fn(name, records, out_words, device=0):
    """One named device function per row of `records` (crt_device_fn, include/crt.h): an (n, input words) array of uint32 or float32,
    taken as bits; returns the (n, out_words) results as uint32.  Row i is computed by lane i % 64 of wave i / 64."""
    r = np.asarray(records)
    if r.dtype not in (np.dtype(np.uint32), np.dtype(np.float32), np.dtype(np.int32)):
        raise TypeError("device_fn: records must be uint32, int32 or float32 (they are passed as bits)")
    r = np.ascontiguousarray(r).view(np.uint32)
    if r.ndim == 1:
        r = r.reshape(-1, 1)
    if r.ndim != 2:
        raise ValueError("device_fn: records must be (n, input words)")
    n, in_words = r.shape
    out = np.zeros((max(n, 1), max(int(out_words), 1)), dtype=np.uint32)
    src = r if n else np.zeros((1, max(in_words, 1)), dtype=np.uint32)
    capi.check(capi.lib().crt_device_fn(device, name.encode(), n, capi.ptr(src), in_words, capi.ptr(out), int(out_words)), "crt_device_fn")
    return out[:n, :int(out_words)]


def device_rcp_check(device=0):
    """(mismatches inside the guarded range, mismatches outside it) of the kernels' short reciprocal against
    the division 1.0f / x over all 2^32 inputs (crt_device_rcp_check)."""
    import ctypes as C
    a, b = C.c_uint64(0), C.c_uint64(0)
    capi.check(capi.lib().crt_device_rcp_check(device, C.byref(a), C.byref(b)), "crt_device_rcp_check")
    return int(a.value), int(b.value)


def device_philox(ctr, key, device=0):
    c = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4)
    k = np.ascontiguousarray(key, dtype=np.uint32).reshape(-1, 2)
    out = np.zeros_like(c)
    capi.check(capi.lib().crt_device_philox(device, c.shape[0], capi.ptr(c), capi.ptr(k), capi.ptr(out)),
               "crt_device_philox")
    return out
