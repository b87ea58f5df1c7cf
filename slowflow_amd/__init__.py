"""slowflow_amd -- Python binding (ctypes) of libslowflow_amd.so, the MI355X-native implementation of
slowflow's variational optical-flow refinement path (include/slowflow_amd.h).

This package is plumbing around the C-ABI for tests, bench.py and Python callers.  It contains no
compute and no CPU fallback: if the HIP library is missing or no GPU is usable every call raises.
"""
import ctypes as C
import os
import subprocess
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SFA_LIB") or os.path.join(_HERE, "libslowflow_amd.so")     # SFA_LIB: an experimental build of the same C-ABI (tuning only)
MAX_REF = 8
MOSAIC_TILE = (64, 16)                          # csrc/mosaic.hip: MOS_TX x MOS_TY, the demosaicing kernels' tile of the destination (columns, rows)
MOSAIC_DTYPES = {"float32": 0, "uint8": 1, "uint16": 2}     # sfa_dev_dtype of a host mosaic

_f = C.POINTER(C.c_float)


class SlowflowError(RuntimeError):
    pass


def build(verbose=False):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], capture_output=True, text=True)
    if out.returncode != 0:
        raise SlowflowError("building libslowflow_amd.so failed:\n" + out.stdout + out.stderr)
    if verbose:
        print(out.stdout)
    return LIB_PATH


class Penalty(C.Structure):
    _fields_ = [("id", C.c_int), ("eps", C.c_float), ("trunc", C.c_float)]


class Params(C.Structure):
    """sfa_params: the cfg keys of the path (variational_mt.cpp:173-192, 533-568)."""
    _fields_ = [
        ("S", C.c_int), ("one_direction", C.c_int), ("smoothing", C.c_int), ("dataterm_norm", C.c_int),
        ("niter_alter", C.c_int), ("niter_outer", C.c_int), ("niter_inner", C.c_int), ("niter_solver", C.c_int),
        ("thres_outer", C.c_float), ("thres_inner", C.c_float), ("sor_omega", C.c_float),
        ("alpha", C.c_float), ("gamma", C.c_float), ("delta", C.c_float),
        ("robust_color", Penalty), ("robust_grad", Penalty), ("robust_reg", Penalty),
        ("rho", C.c_float * MAX_REF), ("omega", C.c_float * MAX_REF),
        ("hbit", C.c_int), ("norm_avg", C.c_float * 3), ("norm_std", C.c_float * 3),
        ("occlusion_reasoning", C.c_int), ("layers", C.c_int), ("p_scale", C.c_float), ("presmooth_sigma", C.c_float),
        ("occlusion_penalty", C.c_float), ("occlusion_alpha", C.c_float), ("niter_graphc", C.c_int), ("sor_order", C.c_int),
    ]


class Image(C.Structure):
    """sfa_image == image_t (epic_flow_extended/image.h:17-23)"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("stride", C.c_int), ("data", _f)]


class Params2f(C.Structure):
    """sfa_params_2frame == variational_params_t (variational.h:16-25)"""
    _fields_ = [("alpha", C.c_float), ("gamma", C.c_float), ("delta", C.c_float), ("sigma", C.c_float),
                ("niter_outer", C.c_int), ("niter_inner", C.c_int), ("niter_solver", C.c_int), ("sor_omega", C.c_float)]


class EnergyParams(C.Structure):
    """sfa_energy_params: dense_tracking's energy keys (setDefault, dense_tracking.cpp:118-165) in the C types the reference reads them in"""
    _fields_ = [("acc_jc", C.c_float), ("acc_bc", C.c_float), ("acc_gc", C.c_float), ("acc_occ", C.c_float), ("acc_cv", C.c_double),
                ("acc_temporal_occ", C.c_double), ("occlusion_threshold", C.c_float), ("occlusion_fb_threshold", C.c_float), ("penalty", C.c_int),
                ("penalty_eps", C.c_double), ("weight", C.c_float), ("skip", C.c_int)]


def energy_params(**kw):
    """sfa_energy_params_default (setDefault's values, weight 0, skip 1) with the given fields replaced"""
    p = EnergyParams()
    lib().sfa_energy_params_default(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


class JetSource(C.Structure):
    """sfa_jet_source: where a rate's jet files sit relative to the tracking frames (the planes as read, the crop, the resize factor)"""
    _fields_ = [("sw", C.c_int), ("sh", C.c_int), ("stride", C.c_int), ("x0", C.c_int), ("y0", C.c_int), ("cw", C.c_int), ("ch", C.c_int),
                ("rescale", C.c_float)]

    def target(self):
        """(w, h) = (lrint(cw * (double)rescale), lrint(ch * (double)rescale)), halves to even (cvRound)"""
        r = np.float64(np.float32(self.rescale))
        return int(np.rint(np.float64(self.cw) * r)), int(np.rint(np.float64(self.ch) * r))


def jet_source(sw, sh, stride=None, crop=None, rescale=None, w=None):
    """a JetSource of sw x sh planes (row stride `stride` elements, default sw); crop: None or (x0, y0, cw, ch) (utils.cpp:308-318); the factor is
    `rescale`, or (1.0f * w) / cw for the target width w (dense_tracking.cpp:1142), or 1"""
    x0, y0, cw, ch = crop if crop is not None else (0, 0, sw, sh)
    if rescale is None:
        rescale = np.float32(w) / np.float32(cw) if w is not None else 1.0
    return JetSource(int(sw), int(sh), int(sw if stride is None else stride), int(x0), int(y0), int(cw), int(ch), float(np.float32(rescale)))


class FuseParams(C.Structure):
    """sfa_fuse_params: dense_tracking's fusion keys (setDefault, dense_tracking.cpp:136-152) in the C types the reference reads them in"""
    _fields_ = [("acc_beta", C.c_double), ("acc_spatial_occ", C.c_double), ("traj_sim_method", C.c_int), ("pin_first", C.c_int), ("traj_sim_thres", C.c_double),
                ("trws_eps", C.c_double), ("trws_max_iter", C.c_int), ("skip", C.c_int)]


def fuse_params(**kw):
    """sfa_fuse_params_default (setDefault's values, skip 1) with the given fields replaced"""
    p = FuseParams()
    lib().sfa_fuse_params_default(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


class NeighParams(C.Structure):
    """sfa_neigh_params: the keys of dense_tracking's neighbour proposals (setDefault, dense_tracking.cpp:136-159) and the seed"""
    _fields_ = [("traj_sim_thres", C.c_double), ("traj_sim_method", C.c_int), ("neigh_hyp", C.c_int), ("neigh_hyp_radius", C.c_float),
                ("neigh_skip1", C.c_int), ("neigh_skip2", C.c_int), ("hyp_neigh_tryouts", C.c_int), ("seed", C.c_uint), ("slots", C.c_int), ("perturb_keep", C.c_int)]


def neigh_params(**kw):
    """sfa_neigh_params_default (setDefault's values, seed 0, slots 4, perturb_keep -1 = not set) with the given fields replaced"""
    p = NeighParams()
    lib().sfa_neigh_params_default(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


class TrackAltParams(C.Structure):
    """sfa_track_alt_params: the rounds (acc_alternate) and the proposals' keys of a track job that alternates"""
    _fields_ = [("rounds", C.c_int), ("neigh", NeighParams)]


def track_alt_params(rounds=5, **kw):
    """sfa_track_alt_params_default with `rounds` and the given fields of its NeighParams replaced (slots and traj_sim_* come from the job)"""
    a = TrackAltParams()
    lib().sfa_track_alt_params_default(C.byref(a))
    a.rounds = int(rounds)
    for k, v in kw.items():
        assert hasattr(a.neigh, k), k
        setattr(a.neigh, k, v)
    return a


class HypLists(C.Structure):
    """sfa_hyp_lists: the five host planes of n segments' hypothesis lists of 16 positions"""
    _fields_ = [("U", C.c_void_p), ("V", C.c_void_p), ("energy", C.c_void_p), ("occ_bits", C.c_void_p), ("origin", C.c_void_p)]


LIST_POSITIONS = 16
_LIST_TYPES = (("U", np.float64), ("V", np.float64), ("energy", np.float64), ("occ", np.uint64), ("origin", np.uint8))


def hyp_lists(U, V, energy, occ_bits, origin=None):
    """K <= 16 slots -> a hypothesis list of 16 positions (a dict U, V (n, 16, Jets, gh, gw), energy, occ, origin (n, 16, gh, gw)): slot k at
    position k, origin k unless given, every further position absent (+Inf, zeros)"""
    n, K, J, gh, gw = U.shape
    assert K <= LIST_POSITIONS
    out = dict(U=np.zeros((n, LIST_POSITIONS, J, gh, gw)), V=np.zeros((n, LIST_POSITIONS, J, gh, gw)), energy=np.full((n, LIST_POSITIONS, gh, gw), np.inf),
               occ=np.zeros((n, LIST_POSITIONS, gh, gw), np.uint64), origin=np.zeros((n, LIST_POSITIONS, gh, gw), np.uint8))
    out["U"][:, :K], out["V"][:, :K], out["energy"][:, :K], out["occ"][:, :K] = U, V, energy, occ_bits
    out["origin"][:, :K] = np.arange(K, dtype=np.uint8).reshape(1, K, 1, 1) if origin is None else origin
    return out


def philox4x32_10(ctr, key):
    """sfa_philox4x32_10 on the host (no GPU): counter (4 words), key (2 words) -> 4 words"""
    c, k, o = (C.c_uint * 4)(*ctr), (C.c_uint * 2)(*key), (C.c_uint * 4)()
    lib().sfa_philox4x32_10(c, k, o)
    return list(o)


class EpicParams(C.Structure):
    """sfa_epic_params: epic_params_t's numeric fields (epic_flow_extended/epic.h:6-15), method 0 = LA, 1 = NW"""
    _fields_ = [("method", C.c_int), ("saliency_th", C.c_float), ("pref_nn", C.c_int), ("pref_th", C.c_float), ("nn", C.c_int), ("coef_kernel", C.c_float),
                ("euc", C.c_float)]


def epic_params(method="LA", saliency_th=0.045, pref_nn=25, pref_th=5.0, nn=100, coef_kernel=0.8, euc=0.001):
    """sfa_epic_params with epic_params_default's values (epic.cpp:127-136) unless given; method "LA" / "NW" (or the number the library takes)"""
    method = {"LA": 0, "NW": 1}.get(method, method)
    return EpicParams(int(method), float(saliency_th), int(pref_nn), float(pref_th), int(nn), float(coef_kernel), float(euc))


class TrackParams(C.Structure):
    """sfa_track_params: a resident track job's shape, its rates and the keys of the three stages (include/slowflow_amd.h)"""
    _fields_ = [("n", C.c_int), ("K", C.c_int), ("Jets", C.c_int), ("w", C.c_int), ("h", C.c_int), ("min_fps_idx", C.c_int), ("do_fuse", C.c_int),
                ("use_occlusions", C.c_int), ("r_Jets", C.c_int * 16), ("source", JetSource * 16), ("weight", C.c_float * 16), ("epsilon", C.c_double),
                ("skip", C.c_int), ("discard", C.c_int), ("energy", EnergyParams), ("fuse", FuseParams), ("coef", C.c_float), ("avg", C.c_float * 3),
                ("std_dev", C.c_float * 3), ("hbit", C.c_int)]


def track_params(w, h, Jets, r_Jets, n=1, sources=None, weights=None, energy=None, fuse=None, avg=None, std=None, **kw):
    """sfa_track_params_default with the job's shape filled in: frames w x h, Jets, one entry of r_Jets per rate (K = len(r_Jets)), capacity n.
    sources: None (every rate an identity source of w x h planes with row stride stride_of(w)) or one JetSource (or None) per rate; weights: None
    (weight[r] = r) or one float per rate; energy / fuse: EnergyParams / FuseParams (their skip is ignored: the job's `skip` rules); avg, std: the
    smoothness weight's img_norm_*; the other fields (min_fps_idx, do_fuse, use_occlusions, epsilon, skip, discard, coef, hbit) by keyword."""
    p = TrackParams()
    lib().sfa_track_params_default(C.byref(p))
    K = len(r_Jets)
    assert 1 <= K <= 16, "1 .. 16 rates"
    p.n, p.K, p.Jets, p.w, p.h = int(n), K, int(Jets), int(w), int(h)
    for r in range(K):
        p.r_Jets[r] = int(r_Jets[r])
        src = sources[r] if sources is not None and sources[r] is not None else jet_source(w, h, stride_of(w))
        p.source[r] = src
        if weights is not None:
            p.weight[r] = float(weights[r])
    if energy is not None:
        p.energy = energy
    if fuse is not None:
        p.fuse = fuse
    for k in range(3):
        if avg is not None:
            p.avg[k] = avg[k]
        if std is not None:
            p.std_dev[k] = std[k]
    for k, v in kw.items():
        assert k in ("min_fps_idx", "do_fuse", "use_occlusions", "epsilon", "skip", "discard", "coef", "hbit"), k
        setattr(p, k, v)
    return p


class TrackFillParams(C.Structure):
    """sfa_track_fill_params: what a track job that fills in takes beside its TrackParams (include/slowflow_amd.h)"""
    _fields_ = [("epic_skip", C.c_float), ("min_size", C.c_int), ("epic", EpicParams), ("workspace_bytes", C.c_size_t)]


def track_fill_params(**kw):
    """sfa_track_fill_params_default (epic_skip 2, min_size 100, epic = epic_params(pref_nn=25, nn=160, coef_kernel=1.1), workspace_bytes 0 = half of the
    free device memory at run time) with the given fields replaced; epic: an EpicParams"""
    f = TrackFillParams()
    lib().sfa_track_fill_params_default(C.byref(f))
    for k, v in kw.items():
        assert k in ("epic_skip", "min_size", "epic", "workspace_bytes"), k
        setattr(f, k, v)
    return f


def track_job_bytes(params, fill=None):
    """sfa_track_job_bytes / sfa_track_job_bytes_fill (host only, no GPU): the device bytes a TrackJob of these parameters allocates; fill: None or a
    TrackFillParams (the interpolation's workspace is not part of it)"""
    L = lib()
    L.sfa_track_job_bytes.argtypes = [C.POINTER(TrackParams), C.POINTER(C.c_size_t)]
    L.sfa_track_job_bytes_fill.argtypes = [C.POINTER(TrackParams), C.POINTER(TrackFillParams), C.POINTER(C.c_size_t)]
    b = C.c_size_t()
    name = "sfa_track_job_bytes" if fill is None else "sfa_track_job_bytes_fill"
    rc = L.sfa_track_job_bytes(C.byref(params), C.byref(b)) if fill is None else L.sfa_track_job_bytes_fill(C.byref(params), C.byref(fill), C.byref(b))
    if rc != 0:
        raise SlowflowError("%s: %s" % (name, L.sfa_last_error(None).decode()))
    return b.value


EXPORTS = [
    "sfa_device_count", "sfa_ctx_create", "sfa_ctx_destroy", "sfa_last_error", "sfa_ctx_sync", "sfa_params_default",
    "sfa_variational", "sfa_variational_2frame", "sfa_variational_2frame_batch", "sfa_epic_nearest_seeds_batch", "sfa_epic_nn_stage_ms", "sfa_ctx_set_epic_search", "sfa_epic_nn_search_info", "sfa_epic_interpolate_batch", "sfa_epic_fit_stage_ms", "sfa_epic_batch", "sfa_epic_saliency_batch", "sfa_epic_batch_stage_ms", "sfa_params_2frame_default", "sfa_pair_job_create", "sfa_pair_job_destroy", "sfa_pair_job_upload", "sfa_pair_job_run", "sfa_pair_job_download", "sfa_pair_job_download_system", "sfa_flow_magnitude_quantile", "sfa_quantile_ranks", "sfa_flow_magnitude_quantiles_device", "sfa_accumulate_consistent", "sfa_accumulate_consistent_scaled", "sfa_jet_source_default", "sfa_jet_flow_resample", "sfa_jet_occlusion_decode", "sfa_hypothesis_energies_scaled", "sfa_accumulate_grid", "sfa_energy_params_default", "sfa_hypothesis_energies", "sfa_hypothesis_energies_ex", "sfa_dt_smoothness_weight", "sfa_fuse_params_default", "sfa_fuse_hypotheses", "sfa_neigh_params_default", "sfa_prune_hypotheses", "sfa_neighbour_proposals", "sfa_rescore_proposals", "sfa_philox4x32_10", "sfa_philox4x32_10_device", "sfa_consistent_regions", "sfa_fill_samples", "sfa_fill_matches", "sfa_fill_trajectories", "variational", "sfa_compute_one_level", "sfa_normalize", "sfa_sor_coupled", "sfa_sor_red_black", "sor_coupled",
    "sfa_image_warp", "sfa_derivative_stack", "sfa_convolve", "sfa_dpsis_weight", "sfa_smoothness", "sfa_sub_laplacian",
    "sfa_add_data_and_match", "sfa_occlusion_costs", "sfa_grid_cut", "sfa_grid_cut_batch", "sfa_gaussian_blur", "sfa_resize_linear", "sfa_resize_linear_fx", "sfa_gaussian_presmooth", "sfa_pyramid_sizes",
    "sfa_pyramid_down", "sfa_resize_flow", "sfa_job_download_level_frame",
    "sfa_sequence_create", "sfa_sequence_destroy", "sfa_sequence_upload", "sfa_sequence_download", "sfa_sequence_normalize", "sfa_sequence_frame_sums", "sfa_normalize_statistics", "sfa_sequence_apply_normalization",
    "sfa_job_create", "sfa_job_destroy", "sfa_job_upload", "sfa_job_upload_resident", "sfa_job_reset_flow", "sfa_job_run", "sfa_job_download", "sfa_job_download_occlusions", "sfa_job_keep_alternation_occlusions", "sfa_job_download_alternation_occlusions", "sfa_job_mpix_iters", "sfa_job_device_bytes",
    "sfa_dev_layout_default", "sfa_job_upload_device", "sfa_job_set_flow_device", "sfa_job_download_device", "sfa_job_changes", "sfa_pair_job_upload_device", "sfa_pair_job_set_flow_device", "sfa_pair_job_download_device", "sfa_sequence_upload_device", "sfa_ctx_wait_stream", "sfa_ctx_signal_stream",
    "sfa_demosaic_device", "sfa_sequence_upload_mosaic_device", "sfa_sequence_upload_mosaic", "sfa_job_set_raw_weights", "sfa_sequence_rescale",
    "sfa_rgb8_to_lab_device", "sfa_sequence_lab", "sfa_epic_job_create", "sfa_epic_job_destroy", "sfa_epic_job_upload", "sfa_epic_job_set_lab", "sfa_epic_job_upload_device", "sfa_epic_job_set_matches_device", "sfa_epic_job_run", "sfa_epic_job_download", "sfa_epic_job_upload_flow", "sfa_epic_job_download_device", "sfa_job_set_flow_epic",
    "sfa_reference_grid", "sfa_reference_taps", "sfa_reference_lab_device", "sfa_reference_lab",
    "sfa_sor_batch_create", "sfa_sor_batch_destroy", "sfa_sor_batch_upload", "sfa_sor_batch_run", "sfa_sor_batch_download",
    "sfa_track_params_default", "sfa_track_job_bytes", "sfa_track_job_create", "sfa_track_job_destroy", "sfa_track_job_upload_flows", "sfa_track_job_upload_frames", "sfa_track_job_upload_flows_device", "sfa_track_job_upload_frames_device", "sfa_track_job_run", "sfa_track_job_download_rate", "sfa_track_job_download_fused", "sfa_track_job_download_best", "sfa_ctx_free_bytes", "sfa_track_job_download_device", "sfa_track_job_stage_ms", "sfa_track_job_upload_occlusions_device", "sfa_track_job_download_rate_device", "sfa_track_job_download_best_device",
    "sfa_track_fill_params_default", "sfa_track_job_bytes_fill", "sfa_track_job_create_fill", "sfa_track_job_upload_fill", "sfa_track_job_upload_fill_device", "sfa_track_job_upload_fill_reference", "sfa_track_job_upload_fill_reference_device", "sfa_track_job_download_fill", "sfa_track_job_fill_ms", "sfa_track_job_fill_info",
    "sfa_track_alt_params_default", "sfa_track_job_bytes_alternate", "sfa_track_job_create_alternate", "sfa_track_job_set_sequence_starts", "sfa_track_job_download_alternation",
    "sfa_division_chain", "sfa_ctx_set_wait_bound", "sfa_debug_set", "sfa_ctx_set_verbose", "sfa_profile_enable", "sfa_profile_read", "sfa_profile_read_kernels", "sfa_timer_start", "sfa_timer_stop",
]

_lib = None


def lib():
    """The loaded C-ABI library.  Fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SlowflowError(f"{LIB_PATH} is missing: build it with slowflow_amd.build() / make -C slowflow_amd/csrc "
                                "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.sfa_last_error.restype = C.c_char_p
        L.sfa_last_error.argtypes = [C.c_void_p]
        L.sfa_job_mpix_iters.restype = C.c_double
        L.sfa_job_mpix_iters.argtypes = [C.c_void_p]
        L.sfa_job_device_bytes.restype = C.c_double
        L.sfa_job_device_bytes.argtypes = [C.c_void_p]
        for name in ("sfa_ctx_destroy", "sfa_job_destroy", "sfa_pair_job_destroy", "sfa_track_job_destroy", "sfa_sor_batch_destroy", "sfa_sequence_destroy", "sfa_epic_job_destroy"):
            if hasattr(L, name):                # an SFA_LIB build of an earlier C-ABI (tools/bench_track.py's baseline) lacks the newest object
                getattr(L, name).restype = None
                getattr(L, name).argtypes = [C.c_void_p]
        _lib = L
    return _lib


def fptr(a):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"], "fp32 C-contiguous planes only"
    return a.ctypes.data_as(_f)


def stride_of(w):
    return ((w + 3) // 4) * 4


def pyramid_sizes(w, h, layers, p_scale):
    """level sizes of the coarse-to-fine pyramid (variational_mt.cpp:576-652); pure host logic, no GPU needed"""
    ws, hs = (C.c_int * 64)(), (C.c_int * 64)()
    n = lib().sfa_pyramid_sizes(int(w), int(h), int(layers), C.c_float(p_scale), ws, hs)
    return list(ws[:n]), list(hs[:n])


def quantile_ranks(N, q):
    """the rank rule of adaptiveFR.cpp:660-666 (sfa_quantile_ranks; host only, no GPU): (k0, k1, average) -- the quantile is the mean of the sorted
    values k0 and k1 when average, else value k0"""
    L = lib()
    L.sfa_quantile_ranks.argtypes = [C.c_size_t, C.c_float, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    k0, k1, av = C.c_size_t(), C.c_size_t(), C.c_int()
    rc = L.sfa_quantile_ranks(int(N), q, C.byref(k0), C.byref(k1), C.byref(av))
    if rc != 0:
        raise SlowflowError("sfa_quantile_ranks(%d, %r): %s" % (N, q, L.sfa_last_error(None).decode()))
    return k0.value, k1.value, bool(av.value)


def accumulate_grid(w, h, skip):
    """the accumulation grid of utils.cpp:522-526 (sfa_accumulate_grid; host only, no GPU): (gw, gh); grid pixel (x, y) sits on image pixel
    (x * (skip + 1) + int(0.5 * skip), y * (skip + 1) + int(0.5 * skip))"""
    L = lib()
    L.sfa_accumulate_grid.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    gw, gh = C.c_int(), C.c_int()
    rc = L.sfa_accumulate_grid(int(w), int(h), int(skip), C.byref(gw), C.byref(gh))
    if rc != 0:
        raise SlowflowError("sfa_accumulate_grid(%d, %d, %d): %s" % (w, h, skip, L.sfa_last_error(None).decode()))
    return gw.value, gh.value


def fill_samples(extent, epic_skip):
    """the sample columns (rows) of the fill-in's matches (sfa_fill_samples; host only, no GPU): the reference's loop `for (int x = floor(0.5f *
    epic_skip); x < extent; x += epic_skip)` with its float step, as an int32 array"""
    L = lib()
    L.sfa_fill_samples.argtypes = [C.c_int, C.c_float, C.c_void_p, C.POINTER(C.c_int)]
    out, c = np.zeros(max(int(extent), 1), np.int32), C.c_int()
    rc = L.sfa_fill_samples(int(extent), float(epic_skip), out.ctypes.data, C.byref(c))
    if rc != 0:
        raise SlowflowError("sfa_fill_samples(%d, %r): %s" % (extent, epic_skip, L.sfa_last_error(None).decode()))
    return out[:c.value].copy()


def reference_grid(w, h, skip):
    """the grid of dense_tracking's reduced reference image (sfa_reference_grid; host only, no GPU): accumulate_grid's (gw, gh), refused where skip is not
    served (0, 1 and 3 are) or where OpenCV's resize would round the size to another grid"""
    L = lib()
    L.sfa_reference_grid.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    gw, gh = C.c_int(), C.c_int()
    if L.sfa_reference_grid(int(w), int(h), int(skip), C.byref(gw), C.byref(gh)) != 0:
        raise SlowflowError("sfa_reference_grid(%d, %d, %d): %s" % (w, h, skip, L.sfa_last_error(None).decode()))
    return gw.value, gh.value


def reference_taps(skip):
    """the taps of the reference image's 8-bit Gaussian blur in 8 fractional bits (sfa_reference_taps; host only, no GPU) as an int32 array; skip 0: none"""
    L = lib()
    L.sfa_reference_taps.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    out, n = np.zeros(16, np.int32), C.c_int()
    if L.sfa_reference_taps(int(skip), out.ctypes.data, C.byref(n)) != 0:
        raise SlowflowError("sfa_reference_taps(%d): %s" % (skip, L.sfa_last_error(None).decode()))
    return out[:n.value].copy()


def default_params():
    p = Params()
    lib().sfa_params_default(C.byref(p))
    return p


def debug_set(name, value=None):
    """test / tooling hook (include/slowflow_amd.h: sfa_debug_set): one switch of the library's cross-check and what-if paths, e.g. debug_set("SFA_UNFUSED", 1);
    value None = back to the default.  The library itself reads these names from the environment only under SFA_DEBUG=1."""
    L = lib()
    L.sfa_debug_set.argtypes = [C.c_char_p, C.c_char_p]
    rc = L.sfa_debug_set(name.encode(), None if value is None else str(value).encode())
    if rc != 0:
        raise SlowflowError("sfa_debug_set(%s): %s" % (name, L.sfa_last_error(None).decode()))


class debug_switches:
    """with debug_switches(SFA_UNFUSED=1, SFA_SOR_CHAIN=5): ... -- sets the switches and restores the defaults on exit"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            debug_set(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            debug_set(k, None)
        return False


def device_count():
    return lib().sfa_device_count()


class Context:
    """sfa_ctx: one GPU, one HIP stream."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        self._children = weakref.WeakSet()          # jobs, sequences, solver batches created on this context: they hold device memory and the stream
        rc = lib().sfa_ctx_create(int(device), C.byref(self.h))
        if rc != 0:
            raise SlowflowError(f"sfa_ctx_create({device}) -> {rc}: {lib().sfa_last_error(None).decode()}")

    def close(self):
        """destroys what was created on the context first: the library's objects keep a pointer to it, and the garbage collector (cycles,
        interpreter shutdown) may finalise a context before its jobs"""
        if self.h:
            for child in list(getattr(self, "_children", ())):
                child.close()
            lib().sfa_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise SlowflowError(f"{what} -> {rc}: {lib().sfa_last_error(self.h).decode()}")

    def sync(self):
        self._ck(lib().sfa_ctx_sync(self.h), "sfa_ctx_sync")

    # ---- ordering against a stream of the caller (slowflow_amd/device.py) ------------------------
    def wait_stream(self, stream=None):
        """the context's stream waits for what `stream` holds now (None / 0: the null stream; an int handle; a torch.cuda.Stream)"""
        from . import device
        device.wait_stream(self, stream)

    def signal_stream(self, stream=None):
        """`stream` waits for what the context's stream holds now"""
        from . import device
        device.signal_stream(self, stream)

    # ---- stage entry points (host planes) -------------------------------------------------------
    def image_warp(self, src3, wx, wy, w, factor, want_mask=True):
        _, h, stride = src3.shape
        dst = np.zeros_like(src3)
        mask = np.zeros((h, stride), np.float32) if want_mask else None
        self._ck(lib().sfa_image_warp(self.h, fptr(dst), fptr(mask) if want_mask else None, fptr(src3), fptr(wx), fptr(wy), w, h, stride, int(factor)), "sfa_image_warp")
        return dst, mask

    def derivative_stack(self, I1, I2, w):
        _, h, stride = I1.shape
        out = np.zeros((8, 3, h, stride), np.float32)
        self._ck(lib().sfa_derivative_stack(self.h, fptr(out), fptr(I1), fptr(I2), w, h, stride), "sfa_derivative_stack")
        return out

    def convolve(self, src, w, order, horiz):
        h, stride = src.shape
        dst = np.zeros_like(src)
        self._ck(lib().sfa_convolve(self.h, fptr(dst), fptr(src), w, h, stride, int(order), int(bool(horiz))), "sfa_convolve")
        return dst

    def dpsis_weight(self, im3, w, avg=(0, 0, 0), std=(1, 1, 1), hbit=0, coef=5.0):
        _, h, stride = im3.shape
        dst = np.zeros((h, stride), np.float32)
        a, s = (C.c_float * 3)(*avg), (C.c_float * 3)(*std)
        self._ck(lib().sfa_dpsis_weight(self.h, fptr(dst), fptr(im3), w, h, stride, C.c_float(coef), a, s, int(hbit)), "sfa_dpsis_weight")
        return dst

    def smoothness(self, method, uu, vv, dpsis, w, alpha, reg):
        h, stride = uu.shape
        sh, sv = np.zeros_like(uu), np.zeros_like(uu)
        self._ck(lib().sfa_smoothness(self.h, int(method), fptr(sh), fptr(sv), fptr(uu), fptr(vv), fptr(dpsis), w, h, stride, C.c_float(alpha), C.byref(reg)), "sfa_smoothness")
        return sh, sv

    def sub_laplacian(self, dst, src, wh, wv, w):
        h, stride = src.shape
        self._ck(lib().sfa_sub_laplacian(self.h, fptr(dst), fptr(src), fptr(wh), fptr(wv), w, h, stride), "sfa_sub_laplacian")
        return dst

    def occlusion_costs(self, p, masks, succ1, succ2, ref1, ref2, w):
        """masks: list of 2ref planes; succ1/succ2/ref1/ref2: lists of 2ref colour images (3,h,stride) -> d0, d1"""
        h, stride = masks[0].shape
        d0, d1 = np.zeros((h, stride), np.float32), np.zeros((h, stride), np.float32)
        n = len(masks)
        arr = lambda xs: (_f * n)(*[fptr(x) for x in xs])
        self._ck(lib().sfa_occlusion_costs(self.h, C.byref(p), fptr(d0), fptr(d1), arr(masks), arr(succ1), arr(succ2), arr(ref1), arr(ref2), w, h, stride),
                 "sfa_occlusion_costs")
        return d0, d1

    def grid_cut(self, d0, d1, alpha, w):
        h, stride = d0.shape
        occ = np.zeros((h, stride), np.float32)
        self._ck(lib().sfa_grid_cut(self.h, fptr(occ), fptr(d0), fptr(d1), w, h, stride, C.c_float(alpha)), "sfa_grid_cut")
        return occ

    def grid_cut_batch(self, d0, d1, alpha, w):
        """d0, d1: [nb, h, stride] cost planes of nb independent windows -> [nb, h, stride] labels, cut in one batch of launches"""
        nb, h, stride = d0.shape
        assert d1.shape == d0.shape
        occ = np.zeros((nb, h, stride), np.float32)
        self._ck(lib().sfa_grid_cut_batch(self.h, fptr(occ), fptr(d0), fptr(d1), nb, w, h, stride, C.c_float(alpha)), "sfa_grid_cut_batch")
        return occ

    def add_data(self, sysm, mask, du, dv, D, chw, w, hd, hg, s, dt_norm, color, grad, ref_term=False):
        a11, a12, a22, b1, b2 = sysm
        h, stride = du.shape
        cw = (_f * 3)(fptr(chw[0]), fptr(chw[1]), fptr(chw[2])) if chw is not None else None
        rc = lib().sfa_add_data_and_match(self.h, fptr(a11), fptr(a12), fptr(a22), fptr(b1), fptr(b2), fptr(mask), fptr(du), fptr(dv), fptr(D), cw,
                                          w, h, stride, C.c_float(hd), C.c_float(hg), C.c_float(s), int(bool(ref_term)), int(dt_norm),
                                          C.byref(color), C.byref(grad))
        return rc

    def sor_coupled(self, du, dv, a11, a12, a22, b1, b2, sh, sv, w, iterations, omega, red_black=False):
        """drop-in for sor_coupled (solver.h:11) on host planes; red_black=True: the labelled two-colour mode (a different algorithm)"""
        h, stride = du.shape
        imgs = [Image(w, h, stride, fptr(a)) for a in (du, dv, a11, a12, a22, b1, b2, sh, sv)]
        fn, name = (lib().sfa_sor_red_black, "sfa_sor_red_black") if red_black else (lib().sfa_sor_coupled, "sfa_sor_coupled")
        self._ck(fn(self.h, *[C.byref(i) for i in imgs], int(iterations), C.c_float(omega)), name)

    def gaussian_blur(self, src, w, sigma):
        h, stride = src.shape
        dst = np.zeros_like(src)
        self._ck(lib().sfa_gaussian_blur(self.h, fptr(dst), fptr(src), w, h, stride, C.c_float(sigma)), "sfa_gaussian_blur")
        return dst

    def resize_linear(self, src, sw, dw, dh):
        sh, sstride = src.shape
        dst = np.zeros((dh, stride_of(dw)), np.float32)
        self._ck(lib().sfa_resize_linear(self.h, fptr(dst), dw, dh, stride_of(dw), fptr(src), sw, sh, sstride), "sfa_resize_linear")
        return dst

    def pyramid_down(self, src, sw, dw, dh, sigma):
        """test hook (sfa_pyramid_down): one pyramid step -- blur with sigma, resize to dw x dh -- of src (nb, nplanes, sh, sstride) through the function the
        job's pyramid runs per level.  Returns (dst (nb, nplanes, dh, stride_of(dw)), (fused, td, lds_bytes)): what k_pyr_down ran with, (0, 0, 0) for the two kernels"""
        nb, nplanes, sh, sstride = src.shape
        dst = np.zeros((nb, nplanes, dh, stride_of(dw)), np.float32)
        info = (C.c_int * 3)()
        L = lib()
        L.sfa_pyramid_down.argtypes = [C.c_void_p, _f, C.c_int, C.c_int, C.c_int, _f, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int)]
        self._ck(L.sfa_pyramid_down(self.h, fptr(dst), int(dw), int(dh), stride_of(dw), fptr(src), int(sw), sh, sstride, nplanes, nb, float(sigma), info),
                 "sfa_pyramid_down")
        return dst, tuple(info)

    def resize_flow(self, wx, wy, sw, dw, dh, post_x, post_y):
        """test hook (sfa_resize_flow): the flow's hand-over between pyramid levels (k_resize_flow) on nb fields wx, wy (nb, sh, sstride): resized to dw x dh and
        multiplied by post_x / post_y.  Returns (wx, wy), (nb, dh, stride_of(dw)) each"""
        nb, sh, sstride = wx.shape
        assert wy.shape == wx.shape
        ox, oy = np.zeros((nb, dh, stride_of(dw)), np.float32), np.zeros((nb, dh, stride_of(dw)), np.float32)
        L = lib()
        L.sfa_resize_flow.argtypes = [C.c_void_p, _f, _f, C.c_int, C.c_int, C.c_int, _f, _f, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
        self._ck(L.sfa_resize_flow(self.h, fptr(ox), fptr(oy), int(dw), int(dh), stride_of(dw), fptr(wx), fptr(wy), int(sw), sh, sstride, nb, float(post_x),
                                   float(post_y)), "sfa_resize_flow")
        return ox, oy

    def gaussian_presmooth(self, src, w, sigma):
        h, stride = src.shape
        dst = np.zeros_like(src)
        self._ck(lib().sfa_gaussian_presmooth(self.h, fptr(dst), fptr(src), w, h, stride, C.c_float(sigma)), "sfa_gaussian_presmooth")
        return dst

    def resize_linear_fx(self, src, sw, fx, fy):
        """cv::resize(src, Size(0,0), fx, fy): dsize = round(size * f), source coordinate (dst + .5) / f - .5"""
        sh, sstride = src.shape
        dw, dh = int(round(sw * fx)), int(round(sh * fy))
        dst = np.zeros((dh, stride_of(dw)), np.float32)
        self._ck(lib().sfa_resize_linear_fx(self.h, fptr(dst), dw, dh, stride_of(dw), fptr(src), sw, sh, sstride, C.c_double(fx), C.c_double(fy)),
                 "sfa_resize_linear_fx")
        return dst, dw

    def normalize(self, frames, w):
        F = len(frames)
        _, h, stride = frames[0].shape
        arr = (_f * F)(*[fptr(f) for f in frames])
        avg, std = (C.c_double * 3)(), (C.c_double * 3)()
        self._ck(lib().sfa_normalize(self.h, arr, F, w, h, stride, avg, std), "sfa_normalize")
        return list(avg), list(std)

    # ---- the path --------------------------------------------------------------------------------
    def _run(self, fn, name, p, wx, wy, frames, w, chw, want_occ):
        h, stride = wx.shape
        F = len(frames)
        arr = (_f * F)(*[fptr(f) for f in frames])
        cw = (_f * 3)(fptr(chw[0]), fptr(chw[1]), fptr(chw[2])) if chw is not None else None
        occ = np.zeros((h, stride), np.float32) if want_occ else None
        change = (C.c_float * 2)()
        rc = fn(self.h, C.byref(p), fptr(wx), fptr(wy), w, h, stride, arr, F, cw, fptr(occ) if want_occ else None, change)
        self._ck(rc, name)
        return (change[0], change[1]), occ

    def variational_2frame(self, wx, wy, im1, im2, w, p=None):
        """the reference's original two-frame `variational` (variational.c:101), in place on wx, wy"""
        h, stride = wx.shape
        self._ck(lib().sfa_variational_2frame(self.h, fptr(wx), fptr(wy), w, h, stride, fptr(im1), fptr(im2), C.byref(p) if p is not None else None),
                 "sfa_variational_2frame")

    def variational_2frame_batch(self, wxs, wys, im1s, im2s, w, p=None):
        """n pairs of one size through one launch sequence (sfa_variational_2frame_batch), each refined in place; pair i comes out bit-identical to
        variational_2frame on that pair alone"""
        n = len(wxs)
        h, stride = wxs[0].shape if n else (0, 0)
        for a in list(wxs) + list(wys):
            assert a.shape == (h, stride), "every flow plane of the batch has one shape"
        for a in list(im1s) + list(im2s):
            assert a.shape == (3, h, stride), "every frame of the batch is 3 planes of the flow's shape"
        assert len(wys) == n and len(im1s) == n and len(im2s) == n, "one wx, wy, im1, im2 per pair"
        L = lib()
        L.sfa_variational_2frame_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(_f), C.POINTER(_f), C.c_int, C.c_int, C.c_int, C.POINTER(_f),
                                                   C.POINTER(_f), C.c_void_p]
        arrs = [(_f * max(n, 1))(*[fptr(a) for a in group]) for group in (wxs, wys, im1s, im2s)]
        self._ck(L.sfa_variational_2frame_batch(self.h, n, arrs[0], arrs[1], w, h, stride, arrs[2], arrs[3], C.byref(p) if p is not None else None),
                 "sfa_variational_2frame_batch")

    def epic_nearest_seeds(self, costs, seeds, nn, workspace_bytes=0, with_status=False):
        """EpicFlow's geodesic k nearest seeds of a batch (sfa_epic_nearest_seeds_batch).  costs: n fp32 (h, w) cost maps of one size, euc already added;
        seeds: n int arrays (ns_i, 2) of (x, y); returns (labels, index, dist): lists of int32 (h, w), int32 (ns_i, nn), float32 (ns_i, nn) -- the bits of the
        host's epic_nearest_seeds.  workspace_bytes: the device-memory budget of a sub-batch (0: half of the free memory).  An image that does not fit the
        budget even alone raises, unless with_status: then a fourth list of ints is returned, 1 for such an image (its arrays are None)"""
        n = len(costs)
        costs = [np.ascontiguousarray(c, dtype=np.float32) for c in costs]
        seeds = [np.ascontiguousarray(s, dtype=np.int32).reshape(-1, 2) for s in seeds]
        assert len(seeds) == n, "one seed array per cost map"
        h, w = costs[0].shape if n else (0, 0)
        for c in costs:
            assert c.shape == (h, w), "every cost map of the batch has one shape"
        ns = [len(s) for s in seeds]
        labels = [np.full((h, w), -2, np.int32) for _ in range(n)]
        index = [np.full((max(k, 0), max(int(nn), 0)), -2, np.int32) for k in ns]
        dist = [np.zeros((max(k, 0), max(int(nn), 0)), np.float32) for k in ns]
        L = lib()
        _i = C.POINTER(C.c_int)
        L.sfa_epic_nearest_seeds_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(_f), C.POINTER(_i), _i, C.c_int, C.POINTER(_i), C.POINTER(_i),
                                                   C.POINTER(_f), C.c_size_t, _i]
        k = max(n, 1)
        ip = lambda a: a.ctypes.data_as(_i)
        status = (C.c_int * k)()
        self._ck(L.sfa_epic_nearest_seeds_batch(self.h, n, w, h, (_f * k)(*[fptr(c) for c in costs]), (_i * k)(*[ip(s) for s in seeds]), (C.c_int * k)(*ns),
                                                int(nn), (_i * k)(*[ip(a) for a in labels]), (_i * k)(*[ip(a) for a in index]),
                                                (_f * k)(*[fptr(a) for a in dist]), int(workspace_bytes), status), "sfa_epic_nearest_seeds_batch")
        status = list(status[:n])
        if with_status:
            pick = lambda xs: [None if s else x for x, s in zip(xs, status)]
            return pick(labels), pick(index), pick(dist), status
        if any(status):
            raise SlowflowError("sfa_epic_nearest_seeds_batch: images %s do not fit a workspace of %d bytes" % ([i for i, s in enumerate(status) if s], workspace_bytes))
        return labels, index, dist

    def epic_nn_stage_ms(self):
        """the kernel milliseconds of the last epic_nearest_seeds by group (sfa_epic_nn_stage_ms): seeds, sweeps, graph, search, lists"""
        ms = (C.c_float * 5)()
        self._ck(lib().sfa_epic_nn_stage_ms(self.h, ms), "sfa_epic_nn_stage_ms")
        return dict(zip(("seeds", "sweeps", "graph", "search", "lists"), [float(v) for v in ms]))

    def set_epic_search(self, mode):
        """how the nearest-seeds stage's graph search holds its state (sfa_ctx_set_epic_search): "dense" (the default: ns * ns floats per image, all seeds at
        once) or "compact" (slices of 64-seed workgroups in one shared workspace, dense rows or sparse maps per image).  Same bits either way.  An int is
        passed through as the C constant."""
        if isinstance(mode, str):
            if mode not in ("dense", "compact"):
                raise SlowflowError("set_epic_search: mode = %r (\"dense\" or \"compact\")" % (mode,))
            mode = ("dense", "compact").index(mode)
        self._ck(lib().sfa_ctx_set_epic_search(self.h, int(mode)), "sfa_ctx_set_epic_search")

    def epic_nn_search_info(self):
        """the graph search of the last nearest-seeds stage (sfa_epic_nn_search_info): slices launched, images searched dense, images searched sparse, the
        largest search workspace in bytes"""
        info = (C.c_longlong * 4)()
        self._ck(lib().sfa_epic_nn_search_info(self.h, info), "sfa_epic_nn_search_info")
        return dict(zip(("slices", "dense", "sparse", "workspace_bytes"), [int(v) for v in info]))

    def epic_interpolate(self, labels, seeds, vects, index, weight, method="LA", stride=None, workspace_bytes=0, with_status=False):
        """EpicFlow's model fit and dense application of a batch (sfa_epic_interpolate_batch).  labels: n int32 (h, w) label maps of one size, or None for
        the models only; seeds: n int arrays (ns_i, 2); vects: n fp32 (ns_i, 2); index, weight: n arrays (ns_i, nn), the nearest-seeds lists with the kernel
        function already applied to the distances; method "LA" or "NW".  Returns (flow_x, flow_y, model): lists of fp32 (h, stride) planes (stride: w unless
        given; columns >= w are not written and hold NaN; None without labels) and fp32 (ns_i, 6) or (ns_i, 2) models -- the bits of the host's
        epic_fit_localaffine / epic_fit_nadarayawatson and epic()'s apply loops.  An image that does not fit workspace_bytes even alone raises, unless
        with_status: then a fourth list of ints is returned, 1 for such an image (its arrays are None)"""
        if method not in ("LA", "NW"):
            raise SlowflowError("epic_interpolate: method %r (LA or NW)" % (method,))
        n = len(seeds)
        seeds = [np.ascontiguousarray(s, dtype=np.int32).reshape(-1, 2) for s in seeds]
        vects = [np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 2) for v in vects]
        index = [np.ascontiguousarray(a, dtype=np.int32) for a in index]
        weight = [np.ascontiguousarray(a, dtype=np.float32) for a in weight]
        assert len(vects) == n and len(index) == n and len(weight) == n, "one array of each kind per image"
        ns = [len(s) for s in seeds]
        nn = index[0].shape[1] if n else 0
        for k in range(n):
            assert len(vects[k]) == ns[k] and index[k].shape == (ns[k], nn) and weight[k].shape == (ns[k], nn), "image %d: vects (ns, 2), index and weight (ns, nn)" % k
        h, w = 1, 1
        if labels is not None:
            labels = [np.ascontiguousarray(a, dtype=np.int32) for a in labels]
            assert len(labels) == n, "one label map per image"
            h, w = labels[0].shape if n else (0, 0)
            for a in labels:
                assert a.shape == (h, w), "every label map of the batch has one shape"
        stride = w if stride is None else int(stride)
        mf = 6 if method == "LA" else 2
        model = [np.zeros((k, mf), np.float32) for k in ns]
        L = lib()
        _i = C.POINTER(C.c_int)
        L.sfa_epic_interpolate_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_i), C.POINTER(_i), C.POINTER(_f), _i, C.c_int, C.POINTER(_i),
                                                 C.POINTER(_f), C.POINTER(_f), C.POINTER(_f), C.c_int, C.POINTER(_f), C.c_size_t, _i]
        k = max(n, 1)
        ip = lambda a: a.ctypes.data_as(_i)
        fx = fy = None
        if labels is not None:
            fx = [np.full((h, max(stride, 0)), np.nan, np.float32) for _ in range(n)]
            fy = [np.full((h, max(stride, 0)), np.nan, np.float32) for _ in range(n)]
        status = (C.c_int * k)()
        self._ck(L.sfa_epic_interpolate_batch(self.h, n, w, h, 0 if method == "LA" else 1, (_i * k)(*[ip(a) for a in labels]) if labels is not None else None,
                                              (_i * k)(*[ip(s) for s in seeds]), (_f * k)(*[fptr(v) for v in vects]), (C.c_int * k)(*ns), int(nn),
                                              (_i * k)(*[ip(a) for a in index]), (_f * k)(*[fptr(a) for a in weight]),
                                              (_f * k)(*[fptr(a) for a in fx]) if fx is not None else None, (_f * k)(*[fptr(a) for a in fy]) if fy is not None else None,
                                              stride, (_f * k)(*[fptr(a) for a in model]), int(workspace_bytes), status), "sfa_epic_interpolate_batch")
        status = list(status[:n])
        if with_status:
            pick = lambda xs: None if xs is None else [None if s else x for x, s in zip(xs, status)]
            return pick(fx), pick(fy), pick(model), status
        if any(status):
            raise SlowflowError("sfa_epic_interpolate_batch: images %s do not fit a workspace of %d bytes" % ([i for i, s in enumerate(status) if s], workspace_bytes))
        return fx, fy, model

    def epic_fit_stage_ms(self):
        """the kernel milliseconds of the last epic_interpolate (sfa_epic_fit_stage_ms): fit, apply"""
        ms = (C.c_float * 2)()
        self._ck(lib().sfa_epic_fit_stage_ms(self.h, ms), "sfa_epic_fit_stage_ms")
        return dict(zip(("fit", "apply"), [float(v) for v in ms]))

    def epic_batch(self, labs, costs, matches, params, workspace_bytes=0, with_status=False, stride=None):
        """epic() for a batch of images of one size as one chain on the GPU (sfa_epic_batch).  labs: n fp32 (3, h, lab_stride) Lab images, or None when
        params.saliency_th == 0; costs: n fp32 (h, w) cost maps, euc already added; matches: n fp32 (nm_i, 4) arrays of x1 y1 x2 y2 (nm_i may be 0); params:
        epic_params(...).  Returns (flow_x, flow_y, rc, counts, kept): lists of fp32 (h, stride) planes (stride: w unless given; columns >= w, and the
        planes of an image with rc 1, hold NaN), epic()'s return values, (3,) int arrays (matches in, after the saliency filter, after the consistency
        filter) and the surviving matches (k, 4).  An image that does not fit workspace_bytes even alone raises, unless with_status: then a sixth list of
        ints is returned, 1 for such an image (its entries in the other lists are None)"""
        n = len(costs)
        costs = [np.ascontiguousarray(c, dtype=np.float32) for c in costs]
        matches = [np.ascontiguousarray(m, dtype=np.float32).reshape(-1, 4) for m in matches]
        assert len(matches) == n, "one match array per cost map"
        h, w = costs[0].shape if n else (0, 0)
        for c in costs:
            assert c.shape == (h, w), "every cost map of the batch has one shape"
        lab_stride = 0
        if labs is not None:
            labs = [np.ascontiguousarray(a, dtype=np.float32) for a in labs]
            assert len(labs) == n, "one Lab image per cost map"
            for a in labs:
                assert a.ndim == 3 and a.shape[:2] == (3, h) and a.shape == labs[0].shape, "Lab images (3, h, lab_stride) of one shape"
            lab_stride = labs[0].shape[2] if n else 0
        stride = w if stride is None else int(stride)
        nm = [len(m) for m in matches]
        fx = [np.full((h, max(stride, 0)), np.nan, np.float32) for _ in range(n)]
        fy = [np.full((h, max(stride, 0)), np.nan, np.float32) for _ in range(n)]
        kept = [np.zeros((max(k, 1), 4), np.float32) for k in nm]
        k = max(n, 1)
        rc = (C.c_int * k)(*([-9] * k))
        counts = ((C.c_int * 3) * k)()
        status = (C.c_int * k)()
        L = lib()
        _i = C.POINTER(C.c_int)
        L.sfa_epic_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(EpicParams), C.POINTER(_f), C.c_int, C.POINTER(_f), C.POINTER(_f), _i,
                                     C.POINTER(_f), C.POINTER(_f), C.c_int, _i, C.POINTER(C.c_int * 3), C.POINTER(_f), C.c_size_t, _i]
        self._ck(L.sfa_epic_batch(self.h, n, w, h, C.byref(params), (_f * k)(*[fptr(a) for a in labs]) if labs is not None else None, lab_stride,
                                  (_f * k)(*[fptr(c) for c in costs]), (_f * k)(*[fptr(m) for m in matches]), (C.c_int * k)(*nm),
                                  (_f * k)(*[fptr(a) for a in fx]), (_f * k)(*[fptr(a) for a in fy]), stride, rc, counts, (_f * k)(*[fptr(a) for a in kept]),
                                  int(workspace_bytes), status), "sfa_epic_batch")
        status = list(status[:n])
        rc = [int(v) for v in rc[:n]]
        counts = [np.array(list(c), np.int32) for c in counts[:n]]
        kept = [a[:int(c[2])] for a, c in zip(kept, counts)]
        if with_status:
            pick = lambda xs: [None if s else x for x, s in zip(xs, status)]
            return pick(fx), pick(fy), pick(rc), pick(counts), pick(kept), status
        if any(status):
            raise SlowflowError("sfa_epic_batch: images %s do not fit a workspace of %d bytes" % ([i for i, s in enumerate(status) if s], workspace_bytes))
        return fx, fy, rc, counts, kept

    def epic_job(self, params, w, h, n=1):
        """a resident EpicFlow batch (sfa_epic_job): n images of w x h, their inputs and fields in GPU memory; params: epic_params(...)"""
        return EpicJob(self, params, w, h, n)

    def epic_saliency(self, labs, sigma_image=0.8, sigma_matrix=1.0, w=None):
        """the saliency of n Lab images (3, h, stride) of one shape (sfa_epic_saliency_batch): n fp32 (h, stride) planes, the bits of the host's saliency(),
        padding columns 0.  w: the images' width inside rows of `stride` floats (None: the whole row)"""
        n = len(labs)
        labs = [np.ascontiguousarray(a, dtype=np.float32) for a in labs]
        for a in labs:
            assert a.ndim == 3 and a.shape[0] == 3 and a.shape == labs[0].shape, "Lab images (3, h, stride) of one shape"
        h, stride = labs[0].shape[1:] if n else (0, 0)
        w = stride if w is None else int(w)
        out = [np.full((h, stride), np.nan, np.float32) for _ in range(n)]
        L = lib()
        L.sfa_epic_saliency_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(_f), C.c_int, C.c_float, C.c_float, C.POINTER(_f)]
        k = max(n, 1)
        self._ck(L.sfa_epic_saliency_batch(self.h, n, w, h, (_f * k)(*[fptr(a) for a in labs]), stride, float(sigma_image), float(sigma_matrix),
                                           (_f * k)(*[fptr(a) for a in out])), "sfa_epic_saliency_batch")
        return out

    def reference_lab(self, rgb, skip, norm=1.0, return_rgb8=False):
        """dense_tracking's reduced reference image of one frame (sfa_reference_lab; dense_tracking.cpp:931-955): rgb fp32 (3, h, w) as read -> the Lab image
        fp32 (3, gh, gw) on the grid of reference_grid(w, h, skip); with return_rgb8 also the reduced 8-bit RGB image uint8 (3, gh, gw)"""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        assert rgb.ndim == 3 and rgb.shape[0] == 3, "rgb is (3, h, w)"
        _, h, w = rgb.shape
        gw, gh = reference_grid(w, h, skip)
        lab = np.zeros((3, gh, gw), np.float32)
        rgb8 = np.zeros((3, gh, gw), np.uint8) if return_rgb8 else None
        L = lib()
        L.sfa_reference_lab.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _f, C.c_int, C.c_float, _f, C.c_int, C.c_void_p]
        self._ck(L.sfa_reference_lab(self.h, w, h, int(skip), fptr(rgb), w, float(norm), fptr(lab), gw, rgb8.ctypes.data if return_rgb8 else None), "sfa_reference_lab")
        return (lab, rgb8) if return_rgb8 else lab

    def epic_batch_stage_ms(self):
        """the kernel milliseconds of the last epic_batch by stage (sfa_epic_batch_stage_ms)"""
        ms = (C.c_float * 8)()
        self._ck(lib().sfa_epic_batch_stage_ms(self.h, ms), "sfa_epic_batch_stage_ms")
        return dict(zip(("saliency", "filters", "nn_prefilter", "estimate", "nn", "weights", "fit", "apply"), [float(v) for v in ms]))

    def flow_magnitude_quantile(self, us, vs, w, flow_scale, q):
        """adaptiveFR's quantile (sfa_flow_magnitude_quantile): the fields' magnitudes after scaling by flow_scale, the rank rule of
        quantile_ranks; returns (quantile, maximum) as floats (doubles)"""
        n = len(us)
        h, stride = us[0].shape if n else (1, max(int(w), 1))
        for a in list(us) + list(vs):
            assert a.shape == (h, stride), "every plane has one shape"
        L = lib()
        L.sfa_flow_magnitude_quantile.argtypes = [C.c_void_p, C.c_int, C.POINTER(_f), C.POINTER(_f), C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]
        ua, va = (_f * max(n, 1))(*[fptr(a) for a in us]), (_f * max(n, 1))(*[fptr(a) for a in vs])
        qv, mv = C.c_double(), C.c_double()
        self._ck(L.sfa_flow_magnitude_quantile(self.h, n, ua, va, w, h, stride, flow_scale, q, C.byref(qv), C.byref(mv)), "sfa_flow_magnitude_quantile")
        return qv.value, mv.value

    def jet_flow_resample(self, u, v, source):
        """sfa_jet_flow_resample: n flow fields u, v, fp32 (n, sh, stride) as `source` (a JetSource) describes them, cropped, resized by
        source.rescale (INTER_LINEAR on doubles) and multiplied by it, on the GPU.  Returns (u, v): float64 (n, h, w), (w, h) = source.target()"""
        u, v = (np.ascontiguousarray(a, dtype=np.float32) for a in (u, v))
        assert u.ndim == 3 and u.shape == v.shape and u.shape[1:] == (source.sh, source.stride), "flows are (n, sh, stride)"
        n = u.shape[0]
        w, h = source.target()
        out_u, out_v = np.zeros((n, h, w), np.float64), np.zeros((n, h, w), np.float64)
        L = lib()
        L.sfa_jet_flow_resample.argtypes = [C.c_void_p, C.c_int, C.POINTER(JetSource), C.POINTER(_f), C.POINTER(_f), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        up, vp = ((_f * max(n, 1))(*[fptr(a[k]) for k in range(n)]) for a in (u, v))
        self._ck(L.sfa_jet_flow_resample(self.h, n, C.byref(source), up, vp, w, h, out_u.ctypes.data, out_v.ctypes.data), "sfa_jet_flow_resample")
        return out_u, out_v

    def jet_occlusion_decode(self, occ, source):
        """sfa_jet_occlusion_decode: n raw occlusion images, uint8 (n, sh, stride), -> masks uint8 (n, h, w), 0 = occluded: INTER_CUBIC resize by
        source.rescale, 3 x 3 median, 255 - x, on the GPU"""
        occ = np.ascontiguousarray(occ, dtype=np.uint8)
        assert occ.ndim == 3 and occ.shape[1:] == (source.sh, source.stride), "occlusion images are (n, sh, stride)"
        n = occ.shape[0]
        w, h = source.target()
        mask = np.zeros((n, h, w), np.uint8)
        L = lib()
        _u8 = C.POINTER(C.c_ubyte)
        L.sfa_jet_occlusion_decode.argtypes = [C.c_void_p, C.c_int, C.POINTER(JetSource), C.POINTER(_u8), C.c_int, C.c_int, C.c_void_p]
        op = (_u8 * max(n, 1))(*[occ[k].ctypes.data_as(_u8) for k in range(n)])
        self._ck(L.sfa_jet_occlusion_decode(self.h, n, C.byref(source), op, w, h, mask.ctypes.data), "sfa_jet_occlusion_decode")
        return mask

    def accumulate_consistent(self, fwd_u, fwd_v, bwd_u, bwd_v, w, epsilon, skip, discard, all_steps=True, masks=None, source=None, stage_ms=None):
        """dense_tracking's accumulateConsistentBatches (sfa_accumulate_consistent) for n segments of FF steps in one call.  fwd_u .. bwd_v: fp32
        arrays (n, FF, h, stride), only the w valid columns read; masks: uint8 (n, FF, h, stride), 0 = occluded, or None.  Returns (acc_u, acc_v,
        tracked): float64 (n, S, gh, gw) with S = FF (all_steps) or 1 (the last step), int32 (n, gh, gw).
        source: a JetSource (sfa_accumulate_consistent_scaled): the flows are (n, FF, sh, source.stride) planes of another size, brought to w x h =
        source.target() on the GPU, and masks are the RAW occlusion images of that shape (decoded on the GPU).  stage_ms: with a source, a list that
        receives the milliseconds of the resampling kernels and of the accumulation kernel"""
        planes = [np.ascontiguousarray(a, dtype=np.float32) for a in (fwd_u, fwd_v, bwd_u, bwd_v)]
        assert planes[0].ndim == 4, "flows are (n, FF, h, stride)"
        n, FF, h, stride = planes[0].shape
        if source is not None:
            assert (h, stride) == (source.sh, source.stride), "flows are (n, FF, source.sh, source.stride)"
            tw, h = source.target()
            assert tw == w, "source.target() is %d wide, not %d" % (tw, w)
        for a in planes:
            assert a.shape == planes[0].shape, "every flow array has one shape"
        if masks is not None:
            masks = np.ascontiguousarray(masks, dtype=np.uint8)
            assert masks.shape == planes[0].shape, "masks have the flows' shape"
        gw, gh = accumulate_grid(w, h, skip) if n and FF else (1, 1)
        S = FF if all_steps else 1
        acc_u, acc_v = np.zeros((n, S, gh, gw), np.float64), np.zeros((n, S, gh, gw), np.float64)
        tracked = np.zeros((n, gh, gw), np.int32)
        L = lib()
        _u8 = C.POINTER(C.c_ubyte)
        L.sfa_accumulate_consistent.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.POINTER(_f)] * 4 + [
            C.POINTER(_u8), C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        k = max(n * FF, 1)
        ptrs = [(_f * k)(*[fptr(a[s, f]) for s in range(n) for f in range(FF)]) for a in planes]
        mp = (_u8 * k)(*[masks[s, f].ctypes.data_as(_u8) for s in range(n) for f in range(FF)]) if masks is not None else None
        if source is not None:
            L.sfa_accumulate_consistent_scaled.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(JetSource)] + [C.POINTER(_f)] * 4 + [
                C.POINTER(_u8), C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
            ms = (C.c_float * 2)()
            self._ck(L.sfa_accumulate_consistent_scaled(self.h, n, FF, w, h, C.byref(source), ptrs[0], ptrs[1], ptrs[2], ptrs[3], mp, C.c_double(epsilon),
                                                        int(skip), int(bool(discard)), int(bool(all_steps)), acc_u.ctypes.data, acc_v.ctypes.data,
                                                        tracked.ctypes.data, ms if stage_ms is not None else None), "sfa_accumulate_consistent_scaled")
            if stage_ms is not None:
                stage_ms[:] = [ms[0], ms[1]]
            return acc_u, acc_v, tracked
        self._ck(L.sfa_accumulate_consistent(self.h, n, FF, w, h, stride, ptrs[0], ptrs[1], ptrs[2], ptrs[3], mp, C.c_double(epsilon), int(skip),
                                             int(bool(discard)), int(bool(all_steps)), acc_u.ctypes.data, acc_v.ctypes.data, tracked.ctypes.data),
                 "sfa_accumulate_consistent")
        return acc_u, acc_v, tracked

    def hypothesis_energies(self, p, r_Jets, acc_u, acc_v, tracked, frames, w, flows=None, adapted=False, flow_source=None):
        """dense_tracking's unary energies (sfa_hypothesis_energies) of every hypothesis of n segments of one rate.  p: EnergyParams; acc_u, acc_v:
        float64 (n, r_Jets, gh, gw) and tracked int32 (n, gh, gw), as accumulate_consistent(all_steps=True) returns them; frames: fp32 (n, Jets + 1,
        3, h, stride) normalised colour frames (c1, c2, c3); flows: None or (fwd_u, fwd_v, bwd_u, bwd_v), fp32 (n, Jets, h, stride) each, rate
        acc_min_fps's flows.  Returns energy float64 (n, gh, gw), +Inf where tracked != r_Jets, and occ_bits uint64 (n, gh, gw), bit t = occluded(t);
        with adapted=True also the flows after adaptFPS(Jets), float64 (n, Jets, gh, gw) each (sfa_hypothesis_energies_ex; 0 without a hypothesis).
        flow_source: a JetSource (sfa_hypothesis_energies_scaled): the flows are (n, Jets, sh, flow_source.stride) planes of another size, brought
        to the frames' size on the GPU"""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        assert frames.ndim == 5 and frames.shape[2] == 3, "frames are (n, Jets + 1, 3, h, stride)"
        n, J1, _, h, stride = frames.shape
        Jets = J1 - 1
        acc_u, acc_v = np.ascontiguousarray(acc_u, dtype=np.float64), np.ascontiguousarray(acc_v, dtype=np.float64)
        tracked = np.ascontiguousarray(tracked, dtype=np.int32)
        gh, gw = tracked.shape[1:]
        assert tracked.shape == (n, gh, gw) and acc_u.shape == (n, r_Jets, gh, gw) and acc_v.shape == acc_u.shape, "acc_u, acc_v, tracked shapes"
        L = lib()
        L.sfa_hypothesis_energies.argtypes = [C.c_void_p, C.POINTER(EnergyParams)] + [C.c_int] * 6 + [C.c_void_p] * 3 + [C.POINTER(_f)] * 5 + [
            C.c_void_p, C.c_void_p]
        fp = (_f * max(n * J1, 1))(*[fptr(frames[s, f]) for s in range(n) for f in range(J1)])
        if flows is not None:
            flows = [np.ascontiguousarray(a, dtype=np.float32) for a in flows]
            for a in flows:
                assert a.shape == ((n, Jets, h, stride) if flow_source is None else (n, Jets, flow_source.sh, flow_source.stride)), "flows are (n, Jets, h, stride)"
            fl = [(_f * max(n * Jets, 1))(*[fptr(a[s, t]) for s in range(n) for t in range(Jets)]) for a in flows]
        else:
            fl = [None] * 4
        energy = np.zeros((n, gh, gw), np.float64)
        occ = np.zeros((n, gh, gw), np.uint64)
        if flow_source is not None:
            L.sfa_hypothesis_energies_scaled.argtypes = [C.c_void_p, C.POINTER(EnergyParams)] + [C.c_int] * 6 + [C.c_void_p] * 3 + [
                C.POINTER(_f), C.POINTER(JetSource)] + [C.POINTER(_f)] * 4 + [C.c_void_p] * 4
            au, av = (np.zeros((n, Jets, gh, gw), np.float64), np.zeros((n, Jets, gh, gw), np.float64)) if adapted else (None, None)
            self._ck(L.sfa_hypothesis_energies_scaled(self.h, C.byref(p), n, int(r_Jets), Jets, w, h, stride, acc_u.ctypes.data, acc_v.ctypes.data,
                                                      tracked.ctypes.data, fp, C.byref(flow_source), fl[0], fl[1], fl[2], fl[3], energy.ctypes.data,
                                                      occ.ctypes.data, au.ctypes.data if adapted else None, av.ctypes.data if adapted else None),
                     "sfa_hypothesis_energies_scaled")
            return (energy, occ, au, av) if adapted else (energy, occ)
        if not adapted:
            self._ck(L.sfa_hypothesis_energies(self.h, C.byref(p), n, int(r_Jets), Jets, w, h, stride, acc_u.ctypes.data, acc_v.ctypes.data, tracked.ctypes.data,
                                               fp, fl[0], fl[1], fl[2], fl[3], energy.ctypes.data, occ.ctypes.data), "sfa_hypothesis_energies")
            return energy, occ
        L.sfa_hypothesis_energies_ex.argtypes = L.sfa_hypothesis_energies.argtypes + [C.c_void_p, C.c_void_p]
        au, av = np.zeros((n, Jets, gh, gw), np.float64), np.zeros((n, Jets, gh, gw), np.float64)
        self._ck(L.sfa_hypothesis_energies_ex(self.h, C.byref(p), n, int(r_Jets), Jets, w, h, stride, acc_u.ctypes.data, acc_v.ctypes.data, tracked.ctypes.data,
                                              fp, fl[0], fl[1], fl[2], fl[3], energy.ctypes.data, occ.ctypes.data, au.ctypes.data, av.ctypes.data),
                 "sfa_hypothesis_energies_ex")
        return energy, occ, au, av

    def smoothness_weight(self, frame0, w, avg=(0, 0, 0), std=(1, 1, 1), hbit=0, coef=5.0):
        """dense_tracking's computeSmoothnessWeight (sfa_dt_smoothness_weight) of one fp32 (3, h, stride) frame: a packed fp32 (h, w) plane"""
        frame0 = np.ascontiguousarray(frame0, dtype=np.float32)
        _, h, stride = frame0.shape
        out = np.zeros((h, w), np.float32)
        L = lib()
        L.sfa_dt_smoothness_weight.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _f, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, _f]
        a, s = (C.c_float * 3)(*avg), (C.c_float * 3)(*std)
        self._ck(L.sfa_dt_smoothness_weight(self.h, int(w), h, stride, fptr(frame0), C.c_float(coef), a, s, int(hbit), fptr(out)), "sfa_dt_smoothness_weight")
        return out

    def fuse_hypotheses(self, p, U, V, energy, occ_bits, weight, w, h, stage_ms=False):
        """dense_tracking's fusion (sfa_fuse_hypotheses) of n segments with K slots.  p: FuseParams; U, V float64 (n, K, Jets, gh, gw) adapted flows;
        energy float64 (n, K, gh, gw), +Inf = no hypothesis; occ_bits uint64 (n, K, gh, gw); weight fp32 (n, h, w) smoothness weights.  Returns a dict:
        slot int32, u, v float64, occ uint8 (n, gh, gw); energy, bound float64 (n,); iters int32 (n,); with stage_ms the 4 kernel stages' ms."""
        U, V = np.ascontiguousarray(U, dtype=np.float64), np.ascontiguousarray(V, dtype=np.float64)
        energy = np.ascontiguousarray(energy, dtype=np.float64)
        occ_bits = np.ascontiguousarray(occ_bits, dtype=np.uint64)
        weight = np.ascontiguousarray(weight, dtype=np.float32)
        n, K, Jets, gh, gw = U.shape
        assert V.shape == U.shape and energy.shape == (n, K, gh, gw) and occ_bits.shape == energy.shape and weight.shape == (n, h, w), "shapes"
        assert accumulate_grid(w, h, p.skip) == (gw, gh), "U, V, energy, occ_bits are not on the grid of (w, h, p.skip)"
        out = dict(slot=np.zeros((n, gh, gw), np.int32), u=np.zeros((n, gh, gw), np.float64), v=np.zeros((n, gh, gw), np.float64),
                   occ=np.zeros((n, gh, gw), np.uint8), energy=np.zeros(n, np.float64), bound=np.zeros(n, np.float64), iters=np.zeros(n, np.int32))
        ms = np.zeros(4, np.float32)
        L = lib()
        L.sfa_fuse_hypotheses.argtypes = [C.c_void_p, C.POINTER(FuseParams)] + [C.c_int] * 5 + [C.c_void_p] * 13
        self._ck(L.sfa_fuse_hypotheses(self.h, C.byref(p), n, K, Jets, int(w), int(h), U.ctypes.data, V.ctypes.data, energy.ctypes.data, occ_bits.ctypes.data,
                                       weight.ctypes.data, out["slot"].ctypes.data, out["u"].ctypes.data, out["v"].ctypes.data, out["occ"].ctypes.data,
                                       out["energy"].ctypes.data, out["bound"].ctypes.data, out["iters"].ctypes.data, ms.ctypes.data if stage_ms else None),
                 "sfa_fuse_hypotheses")
        if stage_ms:
            out["stage_ms"] = ms
        return out

    @staticmethod
    def _lists(d, shape=None):
        """a list dict (hyp_lists) as contiguous arrays of the C types and its sfa_hyp_lists; shape: make an empty one of (n, Jets, gh, gw)"""
        if shape is not None:
            n, J, gh, gw = shape
            d = dict(U=np.zeros((n, LIST_POSITIONS, J, gh, gw)), V=np.zeros((n, LIST_POSITIONS, J, gh, gw)), energy=np.zeros((n, LIST_POSITIONS, gh, gw)),
                     occ=np.zeros((n, LIST_POSITIONS, gh, gw), np.uint64), origin=np.zeros((n, LIST_POSITIONS, gh, gw), np.uint8))
        d = {k: np.ascontiguousarray(d[k], dtype=t) for k, t in _LIST_TYPES}
        n, P, J, gh, gw = d["U"].shape
        assert P == LIST_POSITIONS and d["V"].shape == d["U"].shape, "U, V: (n, 16, Jets, gh, gw)"
        assert all(d[k].shape == (n, P, gh, gw) for k in ("energy", "occ", "origin")), "energy, occ, origin: (n, 16, gh, gw)"
        return d, HypLists(*[d[k].ctypes.data for k, _ in _LIST_TYPES])

    def prune_hypotheses(self, lists, selected, perturb_keep, stage_ms=False):
        """the prune of the alternation's rounds p > 0 (sfa_prune_hypotheses).  lists: a dict as hyp_lists makes it; selected int32 (n, gh, gw): the
        position the last fusion chose, -1 none.  Returns the pruned lists: the selection at position 0, then the best by (float) energy while the
        list holds at most perturb_keep entries; with stage_ms also the 2 kernels' ms."""
        d, hin = self._lists(lists)
        n, _, J, gh, gw = d["U"].shape
        out, hout = self._lists(None, (n, J, gh, gw))
        selected = np.ascontiguousarray(selected, dtype=np.int32)
        assert selected.shape == (n, gh, gw), "selected: (n, gh, gw)"
        L = lib()
        L.sfa_prune_hypotheses.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.POINTER(HypLists), C.POINTER(HypLists), C.c_void_p]
        ms = np.zeros(2, np.float32)
        self._ck(L.sfa_prune_hypotheses(self.h, n, J, gw, gh, int(perturb_keep), selected.ctypes.data, C.byref(hin), C.byref(hout),
                                        ms.ctypes.data if stage_ms else None), "sfa_prune_hypotheses")
        return (out, ms) if stage_ms else out

    def neighbour_proposals(self, p, lists, round, sequence_start, consistent=None, stage_ms=False):
        """the neighbour proposals of one round (sfa_neighbour_proposals).  p: NeighParams; lists: a dict as hyp_lists makes it; sequence_start: one
        uint32 per segment; consistent uint8 (n, gh, gw), needed in round 0.  Returns (lists, src_pixel, src_position, accepted): the lists with the
        accepted proposals at the lowest absent positions; int32 / uint8 (n, 16, gh, gw): the source pixel y * gw + x and position of a position
        filled in this call, -1 / 0 elsewhere; int32 (n,): their count.  With stage_ms a fifth value: the 3 kernels' ms."""
        d, hin = self._lists(lists)
        n, P, J, gh, gw = d["U"].shape
        out, hout = self._lists(None, (n, J, gh, gw))
        seq = np.ascontiguousarray(sequence_start, dtype=np.uint32)
        assert seq.shape == (n,), "sequence_start: one per segment"
        if consistent is not None:
            consistent = np.ascontiguousarray(consistent, dtype=np.uint8)
            assert consistent.shape == (n, gh, gw), "consistent: (n, gh, gw)"
        src_pixel, src_pos, acc = np.zeros((n, P, gh, gw), np.int32), np.zeros((n, P, gh, gw), np.uint8), np.zeros(n, np.int32)
        L = lib()
        L.sfa_neighbour_proposals.argtypes = [C.c_void_p, C.POINTER(NeighParams)] + [C.c_int] * 5 + [C.c_void_p] * 2 + [C.POINTER(HypLists)] * 2 + [C.c_void_p] * 4
        ms = np.zeros(3, np.float32)
        self._ck(L.sfa_neighbour_proposals(self.h, C.byref(p), n, J, gw, gh, int(round), seq.ctypes.data, None if consistent is None else consistent.ctypes.data,
                                           C.byref(hin), C.byref(hout), src_pixel.ctypes.data, src_pos.ctypes.data, acc.ctypes.data,
                                           ms.ctypes.data if stage_ms else None), "sfa_neighbour_proposals")
        return (out, src_pixel, src_pos, acc, ms) if stage_ms else (out, src_pixel, src_pos, acc)

    def rescore_proposals(self, p, lists, src_pixel, frames, w, flows=None, slot_weight=None, stage_ms=False):
        """the accepted proposals of a round scored at their new place (sfa_rescore_proposals).  p: EnergyParams (its weight is ignored); lists,
        src_pixel: as neighbour_proposals returned them; frames fp32 (n, Jets + 1, 3, h, stride); flows: None or (fwd_u, fwd_v, bwd_u, bwd_v), fp32
        (n, Jets, h, stride) each; slot_weight: up to 16 floats, weight_jet_estimation of the rate each slot belongs to (default 0).  Returns the
        lists with energy and occ replaced where src_pixel >= 0; with stage_ms also the scoring launches' ms."""
        d, hl = self._lists(lists)
        d = {k: v.copy() for k, v in d.items()}
        hl = HypLists(*[d[k].ctypes.data for k, _ in _LIST_TYPES])
        n, P, J, gh, gw = d["U"].shape
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        assert frames.ndim == 5 and frames.shape[:3] == (n, J + 1, 3), "frames are (n, Jets + 1, 3, h, stride)"
        h, stride = frames.shape[3:]
        assert accumulate_grid(w, h, p.skip) == (gw, gh), "the lists are not on the grid of (w, h, p.skip)"
        src_pixel = np.ascontiguousarray(src_pixel, dtype=np.int32)
        assert src_pixel.shape == (n, P, gh, gw), "src_pixel: (n, 16, gh, gw)"
        fp = (_f * (n * (J + 1)))(*[fptr(frames[s, f]) for s in range(n) for f in range(J + 1)])
        if flows is not None:
            flows = [np.ascontiguousarray(a, dtype=np.float32) for a in flows]
            for a in flows:
                assert a.shape == (n, J, h, stride), "flows are (n, Jets, h, stride)"
            fl = [(_f * (n * J))(*[fptr(a[s, t]) for s in range(n) for t in range(J)]) for a in flows]
        else:
            fl = [None] * 4
        wt = (C.c_float * LIST_POSITIONS)(*([float(v) for v in slot_weight] if slot_weight is not None else []))
        L = lib()
        L.sfa_rescore_proposals.argtypes = [C.c_void_p, C.POINTER(EnergyParams)] + [C.c_int] * 5 + [C.POINTER(_f)] * 5 + [C.POINTER(C.c_float), C.c_void_p,
                                                                                                                       C.POINTER(HypLists), C.c_void_p]
        ms = np.zeros(1, np.float32)
        self._ck(L.sfa_rescore_proposals(self.h, C.byref(p), n, J, int(w), h, stride, fp, fl[0], fl[1], fl[2], fl[3], wt, src_pixel.ctypes.data, C.byref(hl),
                                         ms.ctypes.data if stage_ms else None), "sfa_rescore_proposals")
        return (d, float(ms[0])) if stage_ms else d

    def philox4x32_10(self, ctr, key):
        """Philox4x32-10 through the device function the proposals' kernel calls: ctr uint32 (n, 4), key uint32 (n, 2) -> uint32 (n, 4)"""
        ctr, key = np.ascontiguousarray(ctr, dtype=np.uint32), np.ascontiguousarray(key, dtype=np.uint32)
        n = ctr.shape[0]
        assert ctr.shape == (n, 4) and key.shape == (n, 2)
        out = np.zeros((n, 4), np.uint32)
        L = lib()
        L.sfa_philox4x32_10_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
        self._ck(L.sfa_philox4x32_10_device(self.h, n, ctr.ctypes.data, key.ctypes.data, out.ctypes.data), "sfa_philox4x32_10_device")
        return out

    def consistent_regions(self, tracked, full, min_size=100):
        """dense_tracking's removeSmallSegments on (tracked == r_Jets) (sfa_consistent_regions) for n maps in one call.  tracked: int32 (n, h, w);
        full: one int per map, its r_Jets.  Returns (mask, kept): uint8 (n, h, w), 1 where tracked == full and the pixel's 4-connected component of
        such pixels has at least min_size pixels, and int32 (n,), the number of 1s"""
        tracked = np.ascontiguousarray(tracked, dtype=np.int32)
        assert tracked.ndim == 3, "tracked is (n, h, w)"
        n, h, w = tracked.shape
        full = np.ascontiguousarray(full, dtype=np.int32).reshape(-1)
        assert len(full) == n, "one entry of full per map"
        mask, kept = np.zeros((n, h, w), np.uint8), np.zeros(max(n, 1), np.int32)
        L = lib()
        L.sfa_consistent_regions.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self._ck(L.sfa_consistent_regions(self.h, n, w, h, tracked.ctypes.data, full.ctypes.data, int(min_size), mask.ctypes.data, kept.ctypes.data),
                 "sfa_consistent_regions")
        return mask, kept[:n]

    def fill_matches(self, acc_u, acc_v, mask, xs, ys, divisor=1):
        """the fill-in's matches (sfa_fill_matches).  acc_u, acc_v: float64 (n, J, h, w) as accumulate_consistent(all_steps=True) returns them; mask:
        uint8 (n, h, w) (consistent_regions); xs, ys: the sample columns and rows (fill_samples); divisor: acc_skip_pixel + 1.  Returns (matches,
        count): fp32 (n, J, len(xs) * len(ys), 4), rows (x, y, x + u / divisor, y + v / divisor) of the samples with mask 1 in raster order, NaN
        behind a map's count (those rows are not written), and int32 (n,)"""
        acc_u, acc_v = np.ascontiguousarray(acc_u, dtype=np.float64), np.ascontiguousarray(acc_v, dtype=np.float64)
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        assert acc_u.ndim == 4 and acc_v.shape == acc_u.shape, "acc_u, acc_v are (n, J, h, w)"
        n, J, h, w = acc_u.shape
        assert mask.shape == (n, h, w), "mask is (n, h, w)"
        xs, ys = np.ascontiguousarray(xs, dtype=np.int32).reshape(-1), np.ascontiguousarray(ys, dtype=np.int32).reshape(-1)
        matches = np.full((n, J, len(xs) * len(ys), 4), np.nan, np.float32)
        count = np.zeros(max(n, 1), np.int32)
        L = lib()
        L.sfa_fill_matches.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self._ck(L.sfa_fill_matches(self.h, n, J, w, h, acc_u.ctypes.data, acc_v.ctypes.data, mask.ctypes.data, xs.ctypes.data, len(xs), ys.ctypes.data,
                                    len(ys), int(divisor), matches.ctypes.data, count.ctypes.data), "sfa_fill_matches")
        return matches, count[:n]

    def fill_trajectories(self, flow_x, flow_y, w, scale=1):
        """the interpolated planes as trajectories (sfa_fill_trajectories).  flow_x, flow_y: fp32 (n, J, h, stride), only the w valid columns read;
        scale: acc_skip_pixel + 1.  Returns (acc_u, acc_v, tracked): float64 (n, J, h, w) = plane * float(scale) widened, int32 (n, h, w) = J -- the
        inputs of hypothesis_energies"""
        flow_x, flow_y = np.ascontiguousarray(flow_x, dtype=np.float32), np.ascontiguousarray(flow_y, dtype=np.float32)
        assert flow_x.ndim == 4 and flow_y.shape == flow_x.shape, "flow_x, flow_y are (n, J, h, stride)"
        n, J, h, stride = flow_x.shape
        w = int(w)
        acc_u, acc_v = np.zeros((n, J, h, max(w, 0)), np.float64), np.zeros((n, J, h, max(w, 0)), np.float64)
        tracked = np.zeros((n, h, max(w, 0)), np.int32)
        L = lib()
        L.sfa_fill_trajectories.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.POINTER(_f), C.POINTER(_f), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        k = max(n * J, 1)
        px, py = ((_f * k)(*[fptr(a[s, j]) for s in range(n) for j in range(J)]) for a in (flow_x, flow_y))
        self._ck(L.sfa_fill_trajectories(self.h, n, J, w, h, stride, px, py, int(scale), acc_u.ctypes.data, acc_v.ctypes.data, tracked.ctypes.data),
                 "sfa_fill_trajectories")
        return acc_u, acc_v, tracked

    def compute_one_level(self, p, wx, wy, frames, w, chw=None, want_occ=False):
        return self._run(lib().sfa_compute_one_level, "sfa_compute_one_level", p, wx, wy, frames, w, chw, want_occ)

    def variational(self, p, wx, wy, frames, w, chw=None, want_occ=False):
        return self._run(lib().sfa_variational, "sfa_variational", p, wx, wy, frames, w, chw, want_occ)

    # ---- profiling / timing ----------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._ck(lib().sfa_profile_enable(self.h, int(on)), "sfa_profile_enable")

    def profile_read(self):
        n, ms, by = C.c_int(), C.c_double(), C.c_double()
        self._ck(lib().sfa_profile_read(self.h, C.byref(n), C.byref(ms), C.byref(by)), "sfa_profile_read")
        return n.value, ms.value, by.value

    def profile_read_kernels(self):
        """(assembly launches, their ms, their pixels x terms, name of the solver kernel shape last launched); call BEFORE profile_enable(False)"""
        n, ms, px = C.c_int(), C.c_double(), C.c_double()
        name = C.create_string_buffer(160)
        self._ck(lib().sfa_profile_read_kernels(self.h, C.byref(n), C.byref(ms), C.byref(px), name, 160), "sfa_profile_read_kernels")
        return n.value, ms.value, px.value, name.value.decode()

    def set_verbose(self, on=True):
        """the reference's per-iteration "avg change" lines on stdout (variational_mt.cpp:404-405, 431-432)"""
        self._ck(lib().sfa_ctx_set_verbose(self.h, int(bool(on))), "sfa_ctx_set_verbose")

    def set_wait_bound(self, spins):
        """test hook: bound of the solver's in-kernel waits in polls (0 = the default of 2^22); see include/slowflow_amd.h"""
        self._ck(lib().sfa_ctx_set_wait_bound(self.h, C.c_uint(int(spins))), "sfa_ctx_set_wait_bound")

    def division_chain(self, a, b):
        """(q_chain, q_exact, admitted) of the shared-reciprocal division test hook (include/slowflow_amd.h: sfa_division_chain)"""
        import numpy as np
        a = np.ascontiguousarray(a, np.float32).ravel(); b = np.ascontiguousarray(b, np.float32).ravel()
        assert a.size == b.size
        qc, qe, ad = np.empty_like(a), np.empty_like(a), np.empty(a.size, np.uint8)
        L = lib()
        L.sfa_division_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        self._ck(L.sfa_division_chain(self.h, a.ctypes.data, b.ctypes.data, qc.ctypes.data, qe.ctypes.data, ad.ctypes.data, a.size), "sfa_division_chain")
        return qc, qe, ad

    def timer_start(self):
        self._ck(lib().sfa_timer_start(self.h), "sfa_timer_start")

    def timer_stop(self):
        ms = C.c_float()
        self._ck(lib().sfa_timer_stop(self.h, C.byref(ms)), "sfa_timer_stop")
        return ms.value


class Job:
    """sfa_job: `batch` frame windows of one size, resident in HBM, refined in lockstep."""

    def __init__(self, ctx, params, w, h, batch=1):
        self.ctx, self.w, self.h, self.batch = ctx, w, h, batch
        self.n_frames = 2 * (params.S - 1) + 1
        self.layers, self.p_scale = params.layers, params.p_scale
        self.h_ = C.c_void_p()
        ctx._ck(lib().sfa_job_create(ctx.h, C.byref(params), w, h, batch, C.byref(self.h_)), "sfa_job_create")
        ctx._children.add(self)

    def upload(self, b, frames, wx=None, wy=None, chw=None):
        F = len(frames)
        _, h, stride = frames[0].shape
        arr = (_f * F)(*[fptr(f) for f in frames])
        cw = (_f * 3)(fptr(chw[0]), fptr(chw[1]), fptr(chw[2])) if chw is not None else None
        self.ctx._ck(lib().sfa_job_upload(self.h_, b, arr, F, fptr(wx) if wx is not None else None, fptr(wy) if wy is not None else None, stride, cw), "sfa_job_upload")

    def upload_resident(self, b, seq, frame_index, wx=None, wy=None, chw=None):
        idx = (C.c_int * len(frame_index))(*frame_index)
        cw = (_f * 3)(fptr(chw[0]), fptr(chw[1]), fptr(chw[2])) if chw is not None else None
        self.ctx._ck(lib().sfa_job_upload_resident(self.h_, b, seq.h_, idx, len(frame_index), fptr(wx) if wx is not None else None,
                                                   fptr(wy) if wy is not None else None, stride_of(self.w), cw), "sfa_job_upload_resident")

    # ---- the device seam (slowflow_amd/device.py): objects with __cuda_array_interface__, asynchronous on the context's stream ----
    def upload_device(self, frames, b0=0, chw=None, channels_last=None):
        """frames [B,F,3,H,W] or [B,F,H,W,3] (fp32 / uint8 / uint16, any strides) in device memory -> windows b0 .. b0 + B - 1"""
        from . import device
        device.job_upload_device(self, frames, b0, chw, channels_last)

    def set_flow_device(self, flow, b0=0, n=None):
        """the initial flow of windows b0 .. from an fp32 device array [B,2,H,W]; None: zeros for n windows (default: all from b0)"""
        from . import device
        device.job_set_flow_device(self, flow, b0, n)

    def download_device(self, out_flow, out_occ=None, b0=0):
        """(u, v) of windows b0 .. b0 + B - 1 into the fp32 device array out_flow [B,2,H,W], the occlusion labels into out_occ [B,H,W]"""
        from . import device
        device.job_download_device(self, out_flow, out_occ, b0)

    def changes(self, b0=0, n=None):
        """the change norms of the last run as a numpy array (n, 2): what download() returns per window, without a download"""
        from . import device
        return device.job_changes(self, b0, n)

    def set_flow_epic(self, epic_job, mul_u=1.0, mul_v=1.0, b0=0, n=None, i0=0):
        """the initial flow of windows b0 .. b0 + n - 1 from the fields of epic_job's images i0 .. (sfa_job_set_flow_epic): resized to the job's size where
        the field's size divides it, then multiplied by mul_u / mul_v (the driver's fx / steps, fy / steps).  n default: every window from b0"""
        n = self.batch - b0 if n is None else n
        L = lib()
        L.sfa_job_set_flow_epic.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float]
        self.ctx._ck(L.sfa_job_set_flow_epic(self.h_, int(b0), int(n), epic_job.h_, int(i0), float(mul_u), float(mul_v)), "sfa_job_set_flow_epic")

    def set_raw_weights(self, red, weight, b0=0, n=None):
        """rawWeighting (utils.cpp:1336-1374) for the windows b0 .. b0 + n - 1 (default: all from b0), formed on the GPU: the bits of passing its planes as
        chw.  red = (red_x, red_y), the cfg's raw_red_loc.  Call it AFTER the window's upload: an upload without chw sets the weights back to ones."""
        n = self.batch - b0 if n is None else n
        L = lib()
        L.sfa_job_set_raw_weights.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]
        self.ctx._ck(L.sfa_job_set_raw_weights(self.h_, int(b0), int(n), int(red[0]), int(red[1]), float(weight)), "sfa_job_set_raw_weights")

    def run(self):
        self.ctx._ck(lib().sfa_job_run(self.h_), "sfa_job_run")

    def download(self, b):
        stride = stride_of(self.w)
        wx, wy = np.zeros((self.h, stride), np.float32), np.zeros((self.h, stride), np.float32)
        change = (C.c_float * 2)()
        self.ctx._ck(lib().sfa_job_download(self.h_, b, fptr(wx), fptr(wy), stride, change), "sfa_job_download")
        return wx, wy, (change[0], change[1])

    def download_occlusions(self, b):
        stride = stride_of(self.w)
        occ = np.zeros((self.h, stride), np.float32)
        self.ctx._ck(lib().sfa_job_download_occlusions(self.h_, b, fptr(occ), stride), "sfa_job_download_occlusions")
        return occ

    def download_level_frame(self, b, level, f, size=None, stride=None):
        """test hook (sfa_job_download_level_frame): frame f of window b at pyramid level `level` as the last run left it, (3, h_level, stride);
        size = (w, h) of the level (default: pyramid_sizes of the job's parameters), stride default stride_of(w)"""
        if size is None:
            ws, hs = pyramid_sizes(self.w, self.h, self.layers, self.p_scale)
            size = (ws[level], hs[level]) if 0 <= level < len(ws) else (self.w, self.h)
        stride = stride_of(size[0]) if stride is None else stride
        out = np.zeros((3, size[1], max(stride, 1)), np.float32)
        L = lib()
        L.sfa_job_download_level_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _f, C.c_int]
        self.ctx._ck(L.sfa_job_download_level_frame(self.h_, int(b), int(level), int(f), fptr(out), int(stride)), "sfa_job_download_level_frame")
        return out

    def keep_alternation_occlusions(self, on=True):
        self.ctx._ck(lib().sfa_job_keep_alternation_occlusions(self.h_, int(on)), "sfa_job_keep_alternation_occlusions")

    def download_alternation_occlusions(self, b, alter):
        stride = stride_of(self.w)
        occ = np.zeros((self.h, stride), np.float32)
        self.ctx._ck(lib().sfa_job_download_alternation_occlusions(self.h_, b, int(alter), fptr(occ), stride), "sfa_job_download_alternation_occlusions")
        return occ

    def mpix_iters(self):
        return lib().sfa_job_mpix_iters(self.h_)

    def device_bytes(self):
        return lib().sfa_job_device_bytes(self.h_)

    def close(self):
        if self.h_:
            if self.ctx.h:                      # a context finalised first (cyclic garbage, interpreter shutdown) took its stream along: nothing to call into
                lib().sfa_job_destroy(self.h_)
            self.h_ = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EpicJob:
    """sfa_epic_job: the inputs of epic() for n images of one size and the fields it leaves, resident in GPU memory.  The job adds params.euc to the cost
    maps itself (cost_has_euc=False), as epic() does on entry."""

    def __init__(self, ctx, params, w, h, n=1):
        self.ctx, self.w, self.h, self.n, self.params = ctx, w, h, n, params
        self.h_ = C.c_void_p()
        L = lib()
        L.sfa_epic_job_create.argtypes = [C.c_void_p, C.POINTER(EpicParams), C.c_int, C.c_int, C.c_int, C.c_void_p]
        ctx._ck(L.sfa_epic_job_create(ctx.h, C.byref(params), int(w), int(h), int(n), C.byref(self.h_)), "sfa_epic_job_create")
        ctx._children.add(self)

    def upload(self, i, matches, edges):
        """image i from host arrays: matches (nm, 4) of x1 y1 x2 y2, edges (h, w) WITHOUT euc"""
        m = np.ascontiguousarray(matches, dtype=np.float32).reshape(-1, 4)
        e = np.ascontiguousarray(edges, dtype=np.float32)
        assert e.shape == (self.h, self.w), "edges: (h, w)"
        L = lib()
        L.sfa_epic_job_upload.argtypes = [C.c_void_p, C.c_int, _f, C.c_int, _f]
        self.ctx._ck(L.sfa_epic_job_upload(self.h_, int(i), fptr(m) if len(m) else None, len(m), fptr(e)), "sfa_epic_job_upload")

    def set_lab(self, lab_seq, frame_index, i0=0):
        """the Lab images of i0 .. from frames of a resident sequence of the job's size (sfa_epic_job_set_lab)"""
        idx = (C.c_int * len(frame_index))(*[int(f) for f in frame_index])
        L = lib()
        L.sfa_epic_job_set_lab.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        self.ctx._ck(L.sfa_epic_job_set_lab(self.h_, int(i0), len(frame_index), lab_seq.h_, idx), "sfa_epic_job_set_lab")

    def upload_device(self, lab=None, cost=None, i0=0, cost_has_euc=False):
        """Lab images [n,3,h,w] and / or cost maps [n,h,w] (fp32, any strides) in device memory -> images i0 .."""
        from . import device
        device.epic_job_upload_device(self, lab, cost, i0, cost_has_euc)

    def set_matches_device(self, i, matches):
        """image i's matches from a contiguous fp32 device array [nm,4]; None or an empty host array: no match"""
        from . import device
        device.epic_job_set_matches_device(self, i, matches)

    def run(self, n=None, workspace_bytes=0, with_status=False):
        """epic() for the images [0, n) (default: all).  Returns (rc, counts): epic()'s values and (n, 3) int32 survivors; waits for the stream.  An image
        that does not fit workspace_bytes even alone raises, unless with_status: then (rc, counts, status)"""
        n = self.n if n is None else int(n)
        k = max(n, 1)
        rc, counts, status = (C.c_int * k)(*([-9] * k)), ((C.c_int * 3) * k)(), (C.c_int * k)()
        L = lib()
        L.sfa_epic_job_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int * 3), C.c_size_t, C.POINTER(C.c_int)]
        self.ctx._ck(L.sfa_epic_job_run(self.h_, n, rc, counts, int(workspace_bytes), status), "sfa_epic_job_run")
        status = [int(v) for v in status[:n]]
        out = [int(v) for v in rc[:n]], np.array([list(c) for c in counts[:n]], np.int32).reshape(n, 3)
        if with_status:
            return out + (status,)
        if any(status):
            raise SlowflowError("sfa_epic_job_run: images %s do not fit a workspace of %d bytes" % ([i for i, s in enumerate(status) if s], workspace_bytes))
        return out

    def download(self, i, stride=None):
        """image i's field as two host planes (h, stride) (stride default w; columns >= w hold NaN)"""
        stride = self.w if stride is None else int(stride)
        fx, fy = np.full((self.h, max(stride, 1)), np.nan, np.float32), np.full((self.h, max(stride, 1)), np.nan, np.float32)
        L = lib()
        L.sfa_epic_job_download.argtypes = [C.c_void_p, C.c_int, _f, _f, C.c_int]
        self.ctx._ck(L.sfa_epic_job_download(self.h_, int(i), fptr(fx), fptr(fy), stride), "sfa_epic_job_download")
        return fx, fy

    def upload_flow(self, i, fx, fy):
        """image i's field from two host planes (h, stride), in place of a run's (sfa_epic_job_upload_flow)"""
        fx, fy = np.ascontiguousarray(fx, dtype=np.float32), np.ascontiguousarray(fy, dtype=np.float32)
        assert fx.shape == fy.shape and fx.shape[0] == self.h, "two planes (h, stride)"
        L = lib()
        L.sfa_epic_job_upload_flow.argtypes = [C.c_void_p, C.c_int, _f, _f, C.c_int]
        self.ctx._ck(L.sfa_epic_job_upload_flow(self.h_, int(i), fptr(fx), fptr(fy), fx.shape[1]), "sfa_epic_job_upload_flow")

    def download_device(self, out_flow, i0=0):
        """the fields of images i0 .. into the fp32 device array out_flow [n,2,h,w]"""
        from . import device
        device.epic_job_download_device(self, out_flow, i0)

    def close(self):
        if self.h_:
            if self.ctx.h:
                lib().sfa_epic_job_destroy(self.h_)
            self.h_ = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PairJob:
    """sfa_pair_job: n frame pairs of one size resident in HBM for the two-frame refinement (variational.c).  run() only enqueues and returns at once;
    download() and Context.sync() wait.  Pair b comes out bit-identical to Context.variational_2frame on that pair alone."""

    def __init__(self, ctx, w, h, n=1, params=None):
        self.ctx, self.w, self.h, self.n = ctx, w, h, n
        self.h_ = C.c_void_p()
        L = lib()
        L.sfa_pair_job_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.sfa_pair_job_upload.argtypes = [C.c_void_p, C.c_int, _f, _f, C.c_int, _f, _f]
        L.sfa_pair_job_run.argtypes = [C.c_void_p]
        L.sfa_pair_job_download.argtypes = [C.c_void_p, C.c_int, _f, _f, C.c_int]
        L.sfa_pair_job_download_system.argtypes = [C.c_void_p, C.c_int, _f, _f, _f, _f, _f, C.c_int]
        ctx._ck(L.sfa_pair_job_create(ctx.h, C.byref(params) if params is not None else None, int(w), int(h), int(n), C.byref(self.h_)), "sfa_pair_job_create")
        ctx._children.add(self)

    def upload(self, b, wx, wy, im1, im2):
        """host planes as for Context.variational_2frame: wx, wy (h, stride), im1, im2 (3, h, stride), one stride"""
        h, stride = wx.shape
        assert h == self.h and wy.shape == (h, stride) and im1.shape == (3, h, stride) and im2.shape == (3, h, stride), "planes of one (h, stride)"
        self.ctx._ck(lib().sfa_pair_job_upload(self.h_, int(b), fptr(wx), fptr(wy), stride, fptr(im1), fptr(im2)), "sfa_pair_job_upload")

    def run(self):
        self.ctx._ck(lib().sfa_pair_job_run(self.h_), "sfa_pair_job_run")

    def download(self, b, stride=None):
        stride = stride_of(self.w) if stride is None else stride
        wx, wy = np.zeros((self.h, stride), np.float32), np.zeros((self.h, stride), np.float32)
        self.ctx._ck(lib().sfa_pair_job_download(self.h_, int(b), fptr(wx), fptr(wy), stride), "sfa_pair_job_download")
        return wx, wy

    def download_system(self, b):
        """test hook: (a11, a12, a22, b1, b2) of pair b as the last run's last data-term launch left them"""
        stride = stride_of(self.w)
        out = [np.zeros((self.h, stride), np.float32) for _ in range(5)]
        self.ctx._ck(lib().sfa_pair_job_download_system(self.h_, int(b), *[fptr(a) for a in out], stride), "sfa_pair_job_download_system")
        return out

    # ---- the device seam (slowflow_amd/device.py): objects with __cuda_array_interface__, asynchronous on the context's stream ----
    def upload_device(self, frames, b0=0, channels_last=None):
        """frames [B,2,3,H,W] or [B,2,H,W,3] (fp32 / uint8 / uint16, any strides) in device memory -> pairs b0 .. b0 + B - 1 (frame 0 = im1)"""
        from . import device
        device.pair_job_upload_device(self, frames, b0, channels_last)

    def set_flow_device(self, flow, b0=0, n=None):
        """the flow of pairs b0 .. from an fp32 device array [B,2,H,W]; None: zeros for n pairs (default: all from b0)"""
        from . import device
        device.pair_job_set_flow_device(self, flow, b0, n)

    def download_device(self, out_flow, b0=0):
        """(u, v) of pairs b0 .. b0 + B - 1 into the fp32 device array out_flow [B,2,H,W]"""
        from . import device
        device.pair_job_download_device(self, out_flow, b0)

    def close(self):
        if self.h_:
            if self.ctx.h:                      # a context finalised first (cyclic garbage, interpreter shutdown) took its stream along: nothing to call into
                lib().sfa_pair_job_destroy(self.h_)
            self.h_ = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrackJob:
    """sfa_track_job: dense_tracking's accumulation, energies and fusion of up to params.n start_jets x params.K rates, resident in HBM.  run() only
    enqueues the whole chain and returns at once; the downloads wait.  Segment s comes out bit-identical to Context.accumulate_consistent(all_steps) ->
    hypothesis_energies(adapted=True) -> smoothness_weight -> fuse_hypotheses on that segment alone.  fill: a TrackFillParams makes it a job that also
    forms every rate's EpicFlow fill-in hypothesis (upload_fill, download_fill) and fuses 2 K slots, slot 2 r + 1 the fill-in of rate r; its run() waits
    where the fill-in reads its counts."""

    def __init__(self, ctx, params, fill=None, alt=None):
        """alt: a TrackAltParams makes it a job that alternates (sfa_track_job_create_alternate): run() does alt.rounds rounds of prune, proposals,
        rescoring and fusion in place of the one fusion; set_sequence_starts, download_alternation"""
        self.ctx, self.params = ctx, TrackParams.from_buffer_copy(params)
        self.fill = TrackFillParams.from_buffer_copy(fill) if fill is not None else None
        self.alt = TrackAltParams.from_buffer_copy(alt) if alt is not None else None
        self.n, self.K, self.Jets, self.w, self.h = params.n, params.K, params.Jets, params.w, params.h
        self.h_ = C.c_void_p()
        L = lib()
        _pf, _u8 = C.POINTER(_f), C.POINTER(C.POINTER(C.c_ubyte))
        L.sfa_track_job_create.argtypes = [C.c_void_p, C.POINTER(TrackParams), C.POINTER(C.c_void_p)]
        L.sfa_track_job_upload_flows.argtypes = [C.c_void_p, C.c_int, C.c_int, _pf, _pf, _pf, _pf, _u8]
        L.sfa_track_job_upload_frames.argtypes = [C.c_void_p, C.c_int, _pf, C.c_int]
        L.sfa_track_job_run.argtypes = [C.c_void_p, C.c_int]
        L.sfa_track_job_download_rate.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
        L.sfa_track_job_download_fused.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
        L.sfa_track_job_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.sfa_track_job_create_fill.argtypes = [C.c_void_p, C.POINTER(TrackParams), C.POINTER(TrackFillParams), C.POINTER(C.c_void_p)]
        L.sfa_track_job_upload_fill.argtypes = [C.c_void_p, C.c_int, _f, C.c_int, _f]
        L.sfa_track_job_download_fill.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.sfa_track_job_fill_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.sfa_track_job_create_alternate.argtypes = [C.c_void_p, C.POINTER(TrackParams), C.POINTER(TrackFillParams), C.POINTER(TrackAltParams),
                                                     C.POINTER(C.c_void_p)]
        L.sfa_track_job_set_sequence_starts.argtypes = [C.c_void_p, C.c_void_p]
        L.sfa_track_job_download_alternation.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
        if self.alt is not None:
            ctx._ck(L.sfa_track_job_create_alternate(ctx.h, C.byref(self.params), C.byref(self.fill) if self.fill is not None else None, C.byref(self.alt),
                                                     C.byref(self.h_)), "sfa_track_job_create_alternate")
        elif self.fill is None:
            ctx._ck(L.sfa_track_job_create(ctx.h, C.byref(self.params), C.byref(self.h_)), "sfa_track_job_create")
        else:
            ctx._ck(L.sfa_track_job_create_fill(ctx.h, C.byref(self.params), C.byref(self.fill), C.byref(self.h_)), "sfa_track_job_create_fill")
        self.gw, self.gh = accumulate_grid(self.w, self.h, params.skip)
        ctx._children.add(self)

    def set_sequence_starts(self, sequence_start):
        """a job that alternates: one uint32 per start_jet of the job, the second key word of its draws"""
        seq = np.zeros(self.n, np.uint32)
        seq[:len(sequence_start)] = sequence_start
        self.ctx._ck(lib().sfa_track_job_set_sequence_starts(self.h_, seq.ctypes.data), "sfa_track_job_set_sequence_starts")

    def download_alternation(self, s):
        """a job that alternates: origin uint8 (gh, gw) of the chosen hypotheses (slot it was born in, | 0x80 a proposal, 255 none) and per round
        energy, bound float64, iters, nodes, accepted int32 (rounds,)"""
        R = self.alt.rounds
        out = dict(origin=np.zeros((self.gh, self.gw), np.uint8), energy=np.zeros(R), bound=np.zeros(R), iters=np.zeros(R, np.int32),
                   nodes=np.zeros(R, np.int32), accepted=np.zeros(R, np.int32))
        self.ctx._ck(lib().sfa_track_job_download_alternation(self.h_, int(s), *[out[k].ctypes.data for k in ("origin", "energy", "bound", "iters", "nodes",
                                                                                                               "accepted")]), "sfa_track_job_download_alternation")
        return out

    def upload_flows(self, s, r, fwd_u, fwd_v, bwd_u, bwd_v, occ=None):
        """rate r of segment s: fp32 (r_Jets[r], sh, stride) arrays as params.source[r] describes them; occ: the raw uint8 occlusion images of that
        shape on a job with use_occlusions"""
        src, rJ = self.params.source[r], self.params.r_Jets[r]
        planes = [np.ascontiguousarray(a, dtype=np.float32) for a in (fwd_u, fwd_v, bwd_u, bwd_v)]
        for a in planes:
            assert a.shape == (rJ, src.sh, src.stride), "flows are (r_Jets[r], source.sh, source.stride)"
        ptrs = [(_f * rJ)(*[fptr(a[k]) for k in range(rJ)]) for a in planes]
        op = None
        if occ is not None:
            occ = np.ascontiguousarray(occ, dtype=np.uint8)
            assert occ.shape == (rJ, src.sh, src.stride), "occlusion images have the flows' shape"
            _u8 = C.POINTER(C.c_ubyte)
            op = (_u8 * rJ)(*[occ[k].ctypes.data_as(_u8) for k in range(rJ)])
        self.ctx._ck(lib().sfa_track_job_upload_flows(self.h_, int(s), int(r), ptrs[0], ptrs[1], ptrs[2], ptrs[3], op), "sfa_track_job_upload_flows")

    def upload_frames(self, s, frames):
        """the normalised colour frames of segment s: fp32 (Jets + 1, 3, h, stride)"""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        assert frames.ndim == 4 and frames.shape[:3] == (self.Jets + 1, 3, self.h), "frames are (Jets + 1, 3, h, stride)"
        fp = (_f * (self.Jets + 1))(*[fptr(frames[k]) for k in range(self.Jets + 1)])
        self.ctx._ck(lib().sfa_track_job_upload_frames(self.h_, int(s), fp, frames.shape[3]), "sfa_track_job_upload_frames")

    def upload_fill(self, s, lab, edges):
        """segment s of a fill job: lab = the Lab image at the grid's size, fp32 (3, gh, stride) (None where epic.saliency_th == 0); edges = the edge
        cost map fp32 (gh, gw), euc not added"""
        edges = np.ascontiguousarray(edges, dtype=np.float32)
        assert edges.shape == (self.gh, self.gw), "edges are (gh, gw)"
        stride = 0
        if lab is not None:
            lab = np.ascontiguousarray(lab, dtype=np.float32)
            assert lab.ndim == 3 and lab.shape[:2] == (3, self.gh), "lab is (3, gh, stride)"
            stride = lab.shape[2]
        self.ctx._ck(lib().sfa_track_job_upload_fill(self.h_, int(s), fptr(lab) if lab is not None else None, stride, fptr(edges)), "sfa_track_job_upload_fill")

    def upload_fill_reference(self, s, rgb, edges, norm=1.0):
        """segment s of a fill job from frame 0 itself: rgb = the frame as read, before the normalisation, fp32 (3, h, stride) at the FRAMES' size (None where
        epic.saliency_th == 0); its Lab image at the grid's size is formed on the GPU (Context.reference_lab's kernel).  edges as upload_fill takes them"""
        edges = np.ascontiguousarray(edges, dtype=np.float32)
        assert edges.shape == (self.gh, self.gw), "edges are (gh, gw)"
        stride = 0
        if rgb is not None:
            rgb = np.ascontiguousarray(rgb, dtype=np.float32)
            assert rgb.ndim == 3 and rgb.shape[:2] == (3, self.h), "rgb is (3, h, stride)"
            stride = rgb.shape[2]
        L = lib()
        L.sfa_track_job_upload_fill_reference.argtypes = [C.c_void_p, C.c_int, _f, C.c_int, C.c_float, _f]
        self.ctx._ck(L.sfa_track_job_upload_fill_reference(self.h_, int(s), fptr(rgb) if rgb is not None else None, stride, float(norm), fptr(edges)),
                     "sfa_track_job_upload_fill_reference")

    def download_fill(self, s, r):
        """rate r's fill-in of segment s: a dict of u, v float64 (r_Jets[r], gh, gw), energy float64 and occ_bits uint64 (gh, gw) (slot 2 r + 1), and the
        ints kept_pixels, matches, filled"""
        rJ, g = self.params.r_Jets[r] if 0 <= r < self.K else 1, (self.gh, self.gw)
        out = dict(u=np.zeros((rJ,) + g, np.float64), v=np.zeros((rJ,) + g, np.float64), energy=np.zeros(g, np.float64), occ_bits=np.zeros(g, np.uint64))
        st = (C.c_int * 3)()
        self.ctx._ck(lib().sfa_track_job_download_fill(self.h_, int(s), int(r), *[out[k].ctypes.data for k in ("u", "v", "energy", "occ_bits")], C.addressof(st)),
                     "sfa_track_job_download_fill")
        out.update(kept_pixels=st[0], matches=st[1], filled=st[2])
        return out

    def fill_ms(self):
        """the last run's fill-in times in ms, summed over the rates: regions and matches, edge costs, the interpolation chain, trajectories (waits)"""
        ms = (C.c_float * 4)()
        self.ctx._ck(lib().sfa_track_job_fill_ms(self.h_, ms), "sfa_track_job_fill_ms")
        return list(ms)

    def fill_info(self):
        """(sub-batches of the last run's interpolation that ran to their end, sub-batches cut short by the workspace and run again), over all rates"""
        info = (C.c_int * 2)()
        L = lib()
        L.sfa_track_job_fill_info.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        self.ctx._ck(L.sfa_track_job_fill_info(self.h_, info), "sfa_track_job_fill_info")
        return info[0], info[1]

    # ---- the device seam (slowflow_amd/device.py): objects with __cuda_array_interface__, asynchronous on the context's stream ----
    def upload_fill_device(self, lab, edges, s0=0):
        """lab: fp32 [ns, 3, gh, gw] (None where epic.saliency_th == 0), edges: fp32 [ns, gh, gw] in device memory (any strides) -> segments s0 .."""
        from . import device
        device.track_job_upload_fill_device(self, lab, edges, s0)

    def upload_fill_reference_device(self, rgb, edges, norm=1.0, s0=0):
        """rgb: fp32 [ns, 3, h, w], frame 0 of each start_jet as read (None where epic.saliency_th == 0), edges: fp32 [ns, gh, gw] in device memory (any
        strides) -> segments s0 ..; the Lab images are formed on the grid in GPU memory"""
        from . import device
        device.track_job_upload_fill_reference_device(self, rgb, edges, norm, s0)

    def upload_flows_device(self, r, fwd, bwd, s0=0):
        """fwd, bwd: fp32 [ns, r_Jets[r], 2, sh, sw] in device memory (any strides) -> rate r of segments s0 .. s0 + ns - 1"""
        from . import device
        device.track_job_upload_flows_device(self, r, fwd, bwd, s0)

    def upload_frames_device(self, frames, s0=0):
        """frames: fp32 [ns, Jets + 1, 3, h, w] in device memory (any strides) -> segments s0 .. s0 + ns - 1"""
        from . import device
        device.track_job_upload_frames_device(self, frames, s0)

    def download_device(self, flow, slot=None, occ=None, stats=None, s0=0):
        """the fused results of segments s0 .. into device arrays: flow float64 [ns, 2, gh, gw] (any strides); contiguous slot int32 [ns, gh, gw], occ
        uint8 [ns, gh, gw], stats float64 [ns, 3]"""
        from . import device
        device.track_job_download_device(self, flow, slot, occ, stats, s0)

    def upload_occlusions_device(self, r, occ, s0=0):
        """occ: [ns, r_Jets[r], sh, sw] in device memory (any strides), uint8 (the raw occlusion images) or float32 (the labels a refinement leaves,
        turned into the driver's grey image) -> the masks of rate r of segments s0 .. s0 + ns - 1, on a job with use_occlusions"""
        from . import device
        device.track_job_upload_occlusions_device(self, r, occ, s0)

    def download_rate_device(self, r, acc=None, tracked=None, energy=None, occ_bits=None, occluded=None, s0=0):
        """rate r of segments s0 .. into device arrays, the values of download_rate: acc float64 [ns, 2, gh, gw] (any strides; the last accumulated
        step); contiguous [ns, gh, gw] tracked int32, energy float64, occ_bits uint64 (or int64), occluded uint8.  None skips an output."""
        from . import device
        device.track_job_download_rate_device(self, r, acc, tracked, energy, occ_bits, occluded, s0)

    def download_best_device(self, best, s0=0):
        """best of segments s0 .. into a contiguous uint8 [ns, gh, gw] device array; also on a job with do_fuse 0"""
        from . import device
        device.track_job_download_best_device(self, best, s0)

    def run(self, ns=None):
        self.ctx._ck(lib().sfa_track_job_run(self.h_, int(self.n if ns is None else ns)), "sfa_track_job_run")

    def download_rate(self, s, r):
        """a dict of (gh, gw) arrays: u, v float64 (the last accumulated step), tracked int32, energy float64, occ_bits uint64, occluded uint8"""
        g = (self.gh, self.gw)
        out = dict(u=np.zeros(g, np.float64), v=np.zeros(g, np.float64), tracked=np.zeros(g, np.int32), energy=np.zeros(g, np.float64),
                   occ_bits=np.zeros(g, np.uint64), occluded=np.zeros(g, np.uint8))
        self.ctx._ck(lib().sfa_track_job_download_rate(self.h_, int(s), int(r), *[out[k].ctypes.data for k in ("u", "v", "tracked", "energy", "occ_bits", "occluded")]),
                     "sfa_track_job_download_rate")
        return out

    def download_fused(self, s):
        """a dict: slot int32, u, v float64, occ, best uint8 (gh, gw); energy, bound (floats), iters (int)"""
        g = (self.gh, self.gw)
        out = dict(slot=np.zeros(g, np.int32), u=np.zeros(g, np.float64), v=np.zeros(g, np.float64), occ=np.zeros(g, np.uint8), best=np.zeros(g, np.uint8))
        e, b, it = C.c_double(), C.c_double(), C.c_int()
        self.ctx._ck(lib().sfa_track_job_download_fused(self.h_, int(s), *[out[k].ctypes.data for k in ("slot", "u", "v", "occ", "best")], C.addressof(e),
                                                        C.addressof(b), C.addressof(it)), "sfa_track_job_download_fused")
        out.update(energy=e.value, bound=b.value, iters=it.value)
        return out

    def download_best(self, s):
        """best uint8 (gh, gw) of segment s: the rate of the lowest fp32 energy, 255 for none; also on a job with do_fuse 0"""
        best = np.zeros((self.gh, self.gw), np.uint8)
        L = lib()
        L.sfa_track_job_download_best.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self.ctx._ck(L.sfa_track_job_download_best(self.h_, int(s), best.ctypes.data), "sfa_track_job_download_best")
        return best

    def stage_ms(self):
        """the last run's kernel times in ms: records, accumulation, energies, weight, labels, pairwise, TRW-S, output (waits for the run)"""
        ms = (C.c_float * 8)()
        self.ctx._ck(lib().sfa_track_job_stage_ms(self.h_, ms), "sfa_track_job_stage_ms")
        return list(ms)

    def close(self):
        if self.h_:
            if self.ctx.h:                      # a context finalised first (cyclic garbage, interpreter shutdown) took its stream along: nothing to call into
                lib().sfa_track_job_destroy(self.h_)
            self.h_ = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def normalize_statistics(sums, w, h):
    """normalize()'s (avg, std) from per-frame sums in frame order (include/slowflow_amd.h: sfa_normalize_statistics; host arithmetic)"""
    s = np.ascontiguousarray(sums, np.float64)
    avg, std = (C.c_double * 3)(), (C.c_double * 3)()
    rc = lib().sfa_normalize_statistics(C.c_void_p(s.ctypes.data), int(s.shape[0]), int(w), int(h), avg, std)
    if rc != 0:
        raise SlowflowError("sfa_normalize_statistics: bad arguments")
    return list(avg), list(std)


class Sequence:
    """sfa_sequence: the frames of a sequence resident on the GPU, normalised there"""

    def __init__(self, ctx, w, h, n):
        self.ctx, self.w, self.h, self.n = ctx, w, h, n
        self.h_ = C.c_void_p()
        ctx._ck(lib().sfa_sequence_create(ctx.h, w, h, n, C.byref(self.h_)), "sfa_sequence_create")
        ctx._children.add(self)

    def upload(self, f, frame3):
        self.ctx._ck(lib().sfa_sequence_upload(self.h_, f, fptr(frame3), frame3.shape[2]), "sfa_sequence_upload")

    def upload_device(self, frames, f0=0, channels_last=None):
        """frames [N,3,H,W] or [N,H,W,3] in device memory -> sequence frames f0 .. f0 + N - 1 (slowflow_amd/device.py); asynchronous"""
        from . import device
        device.sequence_upload_device(self, frames, f0, channels_last)

    def upload_mosaic(self, f, mosaic, red=(1, 0), method=0, origin=(0, 0)):
        """a HOST Bayer mosaic (numpy [H,W], float32 / uint8 / uint16, rows contiguous) -> sequence frame f, demosaiced on the GPU (method 0: bayer2rgbGR,
        2: the 8-bit OpenCV conversion; red = raw_red_loc).  origin = (x0, y0) of the crop of the sequence's size inside the mosaic.  Asynchronous."""
        m = np.asarray(mosaic)
        if m.ndim != 2 or m.dtype.name not in MOSAIC_DTYPES or m.strides[1] != m.itemsize or m.strides[0] % m.itemsize or m.strides[0] < 0:
            raise SlowflowError(f"mosaic: a [H,W] float32 / uint8 / uint16 array with contiguous rows expected, got {m.dtype} {m.shape} strides {m.strides}")
        L = lib()
        L.sfa_sequence_upload_mosaic.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong] + [C.c_int] * 7
        self.ctx._ck(L.sfa_sequence_upload_mosaic(self.h_, int(f), C.c_void_p(m.ctypes.data), MOSAIC_DTYPES[m.dtype.name], m.strides[0] // m.itemsize, m.shape[1],
                                                  m.shape[0], int(origin[0]), int(origin[1]), int(method), int(red[0]), int(red[1])), "sfa_sequence_upload_mosaic")

    def upload_mosaic_device(self, mosaic, red=(1, 0), method=0, f0=0, origin=(0, 0), size=None):
        """mosaics [N,H,W] in device memory (any object with __cuda_array_interface__) -> sequence frames f0 .. f0 + N - 1 (slowflow_amd/device.py); asynchronous"""
        from . import device
        device.sequence_upload_mosaic_device(self, mosaic, red, method, f0, origin, size)

    def rescale_from(self, src, scale, f_dst=0, f_src=0, n=None):
        """the driver's input rescaling of resident frames (sfa_sequence_rescale): src's frames f_src .. blurred (sigma = 1 / sqrt(2 scale)) and resized by
        `scale` into this sequence's frames f_dst ..; this sequence is lrint(w scale) x lrint(h scale).  Asynchronous; both sequences on one context."""
        n = src.n - f_src if n is None else n
        L = lib()
        L.sfa_sequence_rescale.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float]
        self.ctx._ck(L.sfa_sequence_rescale(self.h_, int(f_dst), src.h_, int(f_src), int(n), float(scale)), "sfa_sequence_rescale")

    def lab_from(self, src, norm=1.0, f_dst=0, f_src=0, n=None):
        """the driver's Lab images of resident frames (sfa_sequence_lab): src's frames f_src .. (not yet normalised) times `norm`, rounded to 8 bits and
        converted become this sequence's frames f_dst ..; both sequences of one size on one context"""
        n = min(src.n - f_src, self.n - f_dst) if n is None else n
        L = lib()
        L.sfa_sequence_lab.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float]
        self.ctx._ck(L.sfa_sequence_lab(self.h_, int(f_dst), src.h_, int(f_src), int(n), float(norm)), "sfa_sequence_lab")

    def download(self, f):
        a = np.zeros((3, self.h, stride_of(self.w)), np.float32)
        self.ctx._ck(lib().sfa_sequence_download(self.h_, f, fptr(a), a.shape[2]), "sfa_sequence_download")
        return a

    def normalize(self, f0=0, n=None):
        avg, std = (C.c_double * 3)(), (C.c_double * 3)()
        self.ctx._ck(lib().sfa_sequence_normalize(self.h_, f0, self.n - f0 if n is None else n, avg, std), "sfa_sequence_normalize")
        return list(avg), list(std)

    def frame_sums(self, f0=0, n=None):
        """(n, 6) fp64 sums of the raw frames (per channel: sum, sum of squares)"""
        n = self.n - f0 if n is None else n
        s = np.zeros((n, 6), np.float64)
        self.ctx._ck(lib().sfa_sequence_frame_sums(self.h_, f0, n, C.c_void_p(s.ctypes.data)), "sfa_sequence_frame_sums")
        return s

    def apply_normalization(self, avg, std, f0=0, n=None):
        a, s = (C.c_double * 3)(*avg), (C.c_double * 3)(*std)
        self.ctx._ck(lib().sfa_sequence_apply_normalization(self.h_, f0, self.n - f0 if n is None else n, a, s), "sfa_sequence_apply_normalization")

    def close(self):
        if self.h_:
            if self.ctx.h:                      # a context finalised first (cyclic garbage, interpreter shutdown) took its stream along: nothing to call into
                lib().sfa_sequence_destroy(self.h_)
            self.h_ = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SorBatch:
    """sfa_sor_batch: `batch` independent 2x2-block systems of one size, resident in HBM."""

    def __init__(self, ctx, w, h, batch=1):
        self.ctx, self.w, self.h, self.batch = ctx, w, h, batch
        self.h_ = C.c_void_p()
        ctx._ck(lib().sfa_sor_batch_create(ctx.h, w, h, batch, C.byref(self.h_)), "sfa_sor_batch_create")
        ctx._children.add(self)

    def upload(self, b, du, dv, a11, a12, a22, b1, b2, sh, sv):
        stride = du.shape[1]
        self.ctx._ck(lib().sfa_sor_batch_upload(self.h_, b, *[fptr(a) for a in (du, dv, a11, a12, a22, b1, b2, sh, sv)], stride), "sfa_sor_batch_upload")

    def run(self, iterations, omega):
        self.ctx._ck(lib().sfa_sor_batch_run(self.h_, int(iterations), C.c_float(omega)), "sfa_sor_batch_run")

    def download(self, b):
        stride = stride_of(self.w)
        du, dv = np.zeros((self.h, stride), np.float32), np.zeros((self.h, stride), np.float32)
        self.ctx._ck(lib().sfa_sor_batch_download(self.h_, b, fptr(du), fptr(dv), stride), "sfa_sor_batch_download")
        return du, dv

    def close(self):
        if self.h_:
            if self.ctx.h:                      # a context finalised first (cyclic garbage, interpreter shutdown) took its stream along: nothing to call into
                lib().sfa_sor_batch_destroy(self.h_)
            self.h_ = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
