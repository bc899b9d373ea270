"""ctypes binding of libsteinhip.so (the C ABI declared in include/steinhip.h).

There is no CPU fallback: if the shared library is missing or a call fails, an
exception is raised.  Device pointers are taken from PyTorch-ROCm tensors with
``.data_ptr()``; PyTorch is used for device memory and streams only.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsteinhip.so")

OK, E_BADARG, E_SHAPE, E_WORKSPACE, E_HIP, E_RCCL, E_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6
F32, BF16, F64 = 0, 1, 2

WS_ROWNORM, WS_DIST, WS_HIST, WS_SELECT, WS_PART_G, WS_PART_T, WS_PART_RS, WS_SQPART, WS_SPEC, WS_PLANES = range(10)
WS_NSECTIONS = 10
WSX_LD_DIST, WSX_SPLIT, WSX_SQ_BLOCKS, WSX_HIST_BINS = range(4)
WSX_N = 4
HIST_BINS, HIST_LEVELS = 2048, 3
STAGE_SYMMETRIC = 1
STAGE_UPPER = 2
STAGE_TILES = 4     # distance pass: always the per-tile kernel
STAGE_PANEL = 8     # distance pass: the panel-resident kernel whenever its restrictions hold
FLAG_X3 = 1
FLAG_TIMING = 4
FLAG_TILED = 8
FLAG_NO_WINDOW = 16
FLAG_RANK_WINDOW = 32
FLAG_TILE_DISTANCE = 64
FLAG_TIMING_CONTRACT = 128
FLAG_FOLD = 512     # the fused call takes the folded contraction (K.W, W = G - theta / h2) wherever it is eligible
FLAG_NO_FOLD = 1024  # ... never takes it
FLAG_KSD = 256      # also the kernelized Stein discrepancy sums: sqnorm is double[3] = |phi|^2, S, S_diag
GLM_LINEAR, GLM_LOGISTIC = 0, 1
SOFTMAX_C_MIN, SOFTMAX_C_MAX, SOFTMAX_F_MAX, SOFTMAX_FC_MAX = 2, 32, 1024, 16384   # STEIN_SOFTMAX_*: the domain of the softmax calls
# STEIN_BNN_CLASS_*: the domain of the network classifier's calls ((n_in + CS) * n_hidden <= W_MAX, CS = n_classes rounded up to 4)
BNN_CLASS_NIN_MAX, BNN_CLASS_C_MIN, BNN_CLASS_C_MAX, BNN_CLASS_H_MAX, BNN_CLASS_W_MAX = 128, 2, 32, 512, 16384
PRED_LINK, PRED_MEAN = 0, 1
PRED_RANKS_MAX = 8                # STEIN_PRED_RANKS_MAX: order statistics per stein_predict_*_ranks call
MASS_NORMALISED, MASS_COUNTS = 0, 1   # STEIN_MASS_* (stein_predict_rank_masses)
PRED_Y_POINTS_MAX = 8             # STEIN_PRED_Y_POINTS_MAX: points per stein_predict_*_ycdf call
PRED_Y_PASSES_MAX = 12            # STEIN_PRED_Y_PASSES_MAX: refinement passes of a stein_predict_*_yquantiles call
KERNEL_RBF, KERNEL_IMQ = 0, 1     # STEIN_KERNEL_* (stein_thin, stein_ksd_boot, stein_ksd_matmul, stein_weights)
SPEC_TABLE_WORDS = 65544          # uint64 words of the rank-summed window table ...
SPEC_TABLE_OFFSET_WORDS = 1 << 21  # ... which starts 2^21 words into the SPEC section (slots + entry buffer)
SPEC_HIT_OFFSET, SPEC_SKIP_L0_OFFSET = 64 + 28, 64 + 52   # uint32 state words inside the SELECT section
SPEC_NSTEPS_OFFSET, SPEC_NHITS_OFFSET = 64 + 56, 64 + 60   # medians recorded since the predictor started / window hits
FUSE_FOLDED_OFFSET = 128 + 12     # uint32 in the SELECT section: 1 after a fused call that took the folded contraction
SELECT_BYTES = 192                                        # SelState + SpecState + FuseState
COMM_ID_BYTES = 128                                       # STEIN_COMM_ID_BYTES
T_STAGES = ("prepare", "distance", "median", "contract", "finish")   # STEIN_T_* of include/steinhip.h

_c = ctypes
_vp, _i64, _int, _dbl, _sz = _c.c_void_p, _c.c_int64, _c.c_int, _c.c_double, _c.c_size_t

# name -> argtypes; every function returns int except the two noted below
_SIGNATURES = {
    "stein_workspace_bytes": [_i64, _i64, _i64, _int, _int, _c.POINTER(_sz)],
    "stein_workspace_layout": [_i64, _i64, _i64, _int, _int, _c.POINTER(_sz), _c.POINTER(_i64)],
    "stein_layout_folds": [_i64, _i64, _i64, _int, _int, _c.POINTER(_int)],
    "stein_layout_fold_ranges": [_i64, _i64, _i64, _int, _int, _c.POINTER(_int)],
    "stein_debug_fold_split": [_int],
    "stein_debug_no_warm": [_int],
    "stein_spec_begin": [_vp, _vp, _vp, _i64, _vp],
    "stein_distance_block_spec": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _i64, _vp, _vp, _int, _vp, _vp, _vp],
    "stein_spec_tally": [_vp, _vp, _vp],
    "stein_spec_pick": [_vp, _vp, _i64, _vp, _vp, _vp],
    "stein_spec_update": [_vp, _vp],
    "stein_score_glm": [_vp, _i64, _i64, _int, _i64, _i64, _i64, _vp, _vp, _i64, _dbl, _dbl, _dbl, _vp, _vp],
    "stein_score_bnn": [_vp, _i64, _i64, _i64, _i64, _c.POINTER(_i64), _vp, _vp, _i64, _dbl, _dbl, _dbl, _vp, _vp],
    "stein_score_bnn_wide": [_vp, _i64, _i64, _i64, _i64, _c.POINTER(_i64), _vp, _vp, _i64, _dbl, _dbl, _dbl, _vp, _vp],
    "stein_score_softmax": [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _dbl, _dbl, _dbl, _vp, _vp],
    "stein_debug_score_softmax_lanes": [_int],
    "stein_predict_softmax_workspace_bytes": [_i64, _i64, _i64, _c.POINTER(_sz)],
    "stein_predict_softmax": [_vp, _i64, _i64, _int, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "stein_predict_softmax_weighted_workspace_bytes": [_i64, _i64, _i64, _c.POINTER(_sz)],
    "stein_predict_softmax_weighted": [_vp, _i64, _i64, _int, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _sz, _vp],
    "stein_score_bnn_class": [_vp, _i64, _i64, _i64, _i64, _i64, _c.POINTER(_i64), _vp, _vp, _i64, _dbl, _dbl, _dbl, _vp, _vp],
    "stein_predict_bnn_class_workspace_bytes": [_i64, _i64, _i64, _c.POINTER(_sz)],
    "stein_predict_bnn_class": [_vp, _i64, _i64, _int, _i64, _i64, _i64, _c.POINTER(_i64), _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                _vp, _sz, _vp],
    "stein_predict_bnn_class_weighted_workspace_bytes": [_i64, _i64, _i64, _c.POINTER(_sz)],
    "stein_predict_bnn_class_weighted": [_vp, _i64, _i64, _int, _i64, _i64, _i64, _c.POINTER(_i64), _vp, _vp, _i64, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "stein_predict_workspace_bytes": [_i64, _i64, _c.POINTER(_sz)],
    "stein_predict_glm": [_vp, _i64, _i64, _int, _int, _i64, _i64, _vp, _vp, _i64, _dbl, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "stein_predict_bnn": [_vp, _i64, _i64, _i64, _i64, _c.POINTER(_i64), _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "stein_predict_weighted_workspace_bytes": [_i64, _i64, _c.POINTER(_sz)],
    "stein_predict_glm_weighted": [_vp, _i64, _i64, _int, _int, _i64, _i64, _vp, _vp, _i64, _dbl, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _sz, _vp],
    "stein_predict_bnn_weighted": [_vp, _i64, _i64, _i64, _i64, _c.POINTER(_i64), _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _sz, _vp],
    "stein_predict_bnn_wide": [_vp, _i64, _i64, _i64, _i64, _c.POINTER(_i64), _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _sz,
                               _vp],
    "stein_predict_bnn_wide_weighted": [_vp, _i64, _i64, _i64, _i64, _c.POINTER(_i64), _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _sz, _vp],
    "stein_predict_ranks_workspace_bytes": [_i64, _i64, _i64, _c.POINTER(_sz)],
    "stein_predict_glm_ranks": [_vp, _i64, _i64, _int, _int, _i64, _i64, _vp, _i64, _c.POINTER(_i64), _i64, _vp, _vp, _sz, _vp],
    "stein_predict_bnn_ranks": [_vp, _i64, _i64, _i64, _i64, _c.POINTER(_i64), _int, _vp, _i64, _c.POINTER(_i64), _i64, _vp, _vp,
                                _sz, _vp],
    "stein_debug_predict_ranks_slices": [_int],
    "stein_predict_ranks_weighted_workspace_bytes": [_i64, _i64, _i64, _c.POINTER(_sz)],
    "stein_predict_glm_ranks_weighted": [_vp, _i64, _i64, _int, _int, _i64, _i64, _vp, _i64, _vp, _c.POINTER(_dbl), _i64, _vp,
                                         _vp, _sz, _vp],
    "stein_predict_bnn_ranks_weighted": [_vp, _i64, _i64, _i64, _i64, _c.POINTER(_i64), _int, _vp, _i64, _vp, _c.POINTER(_dbl),
                                         _i64, _vp, _vp, _sz, _vp],
    "stein_debug_predict_ranks_weighted_bits": [_int],
    "stein_predict_rank_masses_workspace_bytes": [_i64, _c.POINTER(_sz)],
    "stein_predict_rank_masses": [_vp, _i64, _int, _vp, _vp, _vp, _sz, _vp],
    "stein_predict_ycdf_workspace_bytes": [_i64, _i64, _i64, _c.POINTER(_sz)],
    "stein_predict_yquantiles_workspace_bytes": [_i64, _i64, _i64, _c.POINTER(_sz)],
    "stein_predict_glm_ycdf": [_vp, _i64, _i64, _int, _i64, _i64, _vp, _i64, _dbl, _vp, _i64, _vp, _vp, _vp, _sz, _vp],
    "stein_predict_bnn_ycdf": [_vp, _i64, _i64, _i64, _i64, _c.POINTER(_i64), _vp, _i64, _vp, _i64, _vp, _vp, _vp, _sz, _vp],
    "stein_predict_glm_yquantiles": [_vp, _i64, _i64, _int, _i64, _i64, _vp, _i64, _dbl, _c.POINTER(_dbl), _i64, _int, _vp, _vp,
                                     _vp, _vp, _sz, _vp],
    "stein_predict_bnn_yquantiles": [_vp, _i64, _i64, _i64, _i64, _c.POINTER(_i64), _vp, _i64, _c.POINTER(_dbl), _i64, _int, _vp,
                                     _vp, _vp, _vp, _sz, _vp],
    "stein_rank_begin": [_vp, _i64, _i64, _i64, _i64, _int, _vp, _sz, _int, _vp],
    "stein_rank_pick": [_i64, _i64, _i64, _i64, _int, _vp, _sz, _int, _vp, _vp, _vp, _vp],
    "stein_rank_radix": [_int, _int, _i64, _i64, _i64, _i64, _int, _vp, _sz, _int, _vp, _vp, _vp],
    "stein_rank_finish": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_comm_unique_id": [_vp, _sz],
    "stein_comm_init": [_vp, _sz, _int, _int, _c.POINTER(_vp)],
    "stein_comm_info": [_vp, _c.POINTER(_int), _c.POINTER(_int)],
    "stein_comm_destroy": [_vp],
    "stein_rank_step": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _int,
                        _c.POINTER(_int), _vp],
    "stein_timing_reserve": [_int],
    "stein_timing_read": [_c.POINTER(_c.c_float), _int, _c.POINTER(_int)],
    "stein_svgd_phi": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_stream_workspace_bytes": [_i64, _i64, _int, _int, _c.POINTER(_sz)],
    "stein_stream_plan": [_i64, _i64, _c.POINTER(_int), _c.POINTER(_int), _c.POINTER(_int)],
    "stein_svgd_phi_stream": [_vp, _vp, _i64, _i64, _int, _vp, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_debug_stream_jsplit": [_int],
    "stein_stream_ksd_workspace_bytes": [_i64, _i64, _int, _int, _c.POINTER(_sz)],
    "stein_svgd_phi_stream_ksd": [_vp, _vp, _i64, _i64, _int, _vp, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_stream_median_workspace_bytes": [_i64, _i64, _int, _int, _c.POINTER(_sz)],
    "stein_stream_median_plan": [_i64, _i64, _c.POINTER(_sz), _c.POINTER(_sz), _c.POINTER(_i64), _c.POINTER(_int)],
    "stein_stream_median": [_vp, _i64, _i64, _int, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_debug_stream_median_grid": [_int],
    "stein_imq_workspace_bytes": [_i64, _i64, _int, _int, _c.POINTER(_sz)],
    "stein_imq_ksd_workspace_bytes": [_i64, _i64, _int, _int, _c.POINTER(_sz)],
    "stein_imq_plan": [_i64, _i64, _c.POINTER(_int), _c.POINTER(_int), _c.POINTER(_int)],
    "stein_svgd_phi_imq": [_vp, _vp, _i64, _i64, _int, _vp, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_svgd_phi_imq_ksd": [_vp, _vp, _i64, _i64, _int, _vp, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_thin_workspace_bytes": [_i64, _i64, _int, _int, _c.POINTER(_sz)],
    "stein_thin": [_vp, _vp, _i64, _i64, _int, _vp, _int, _i64, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_debug_thin_grid": [_int],
    "stein_ksd_boot_workspace_bytes": [_i64, _i64, _i64, _int, _int, _c.POINTER(_sz)],
    "stein_ksd_boot_plan": [_i64, _i64, _i64, _c.POINTER(_int), _c.POINTER(_int), _c.POINTER(_int)],
    "stein_ksd_boot": [_vp, _vp, _i64, _i64, _int, _vp, _int, _vp, _i64, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_debug_boot_jsplit": [_int],
    "stein_ksd_matmul_workspace_bytes": [_i64, _i64, _i64, _int, _int, _c.POINTER(_sz)],
    "stein_ksd_matmul": [_vp, _vp, _i64, _i64, _int, _vp, _int, _vp, _i64, _vp, _vp, _sz, _int, _vp],
    "stein_weights_workspace_bytes": [_i64, _i64, _int, _int, _c.POINTER(_sz)],
    "stein_weights": [_vp, _vp, _i64, _i64, _int, _vp, _int, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_debug_weights_grid": [_int],
    "stein_rownorms": [_vp, _i64, _i64, _int, _vp, _vp],
    "stein_distance_block": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _i64, _vp, _vp, _int, _vp],
    "stein_x3_prepare": [_vp, _vp, _i64, _i64, _int, _vp, _sz, _vp],
    "stein_median_begin": [_vp, _vp, _i64, _vp],
    "stein_median_hist_pass": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _int, _vp],
    "stein_median_resolve": [_vp, _int, _i64, _vp, _vp, _vp, _vp],
    "stein_kernel_matrix": [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _int, _vp],
    "stein_kernel_contract": [_vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_contract_partial": [_vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_contract_finish": [_vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _sz, _int, _vp],
    "stein_apply_adagrad": [_vp, _vp, _int, _vp, _i64, _int, _vp, _dbl, _dbl, _dbl, _dbl, _dbl, _int, _vp, _vp],
    "stein_apply_adam": [_vp, _vp, _int, _vp, _vp, _i64, _int, _vp, _dbl, _dbl, _dbl, _dbl, _dbl, _dbl, _i64, _vp, _vp],
    "stein_cast_f64_to_f32": [_vp, _vp, _i64, _vp],
    "stein_cast_f32_to_bf16": [_vp, _vp, _i64, _vp],
    "stein_take_device_error": [],
    "stein_debug_hist_all_grid": [_int],
    "stein_debug_hist_all_vblocks": [_int],
    "stein_debug_raise_device_error": [],
}
EXPORTED_SYMBOLS = sorted(list(_SIGNATURES) + ["stein_version", "stein_last_error"])

_lib = None


class SteinHipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libsteinhip error %d: %s" % (code, message))
        self.code = code


def load():
    """Load the library once.  Raises if it has not been built (python __graft_entry__.py)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libsteinhip.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`. "
            "stein_amd has no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, args in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, _int
    lib.stein_version.argtypes, lib.stein_version.restype = [], _int
    lib.stein_last_error.argtypes, lib.stein_last_error.restype = [], _c.c_char_p
    _lib = lib
    return lib


def check(rc):
    if rc != OK:
        msg = load().stein_last_error().decode("utf-8", "replace")
        if rc in (E_BADARG, E_SHAPE, E_UNSUPPORTED):
            raise ValueError("libsteinhip error %d: %s" % (rc, msg))
        raise SteinHipError(rc, msg)


def call(name, *args):
    check(getattr(load(), name)(*args))


def call_on(device, name, *args):
    """`call` with `device` (a torch.device of type cuda) as the process's current HIP device for its duration.

    The library launches on the caller's stream; stream 0 and kernel attributes belong to the CURRENT device, so a
    tensor on cuda:1 handed over while cuda:0 is current would be launched on the wrong GPU.  The common case (the
    tensor's device is already current) costs one integer comparison.
    """
    import torch
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx == torch.cuda.current_device():
        return call(name, *args)
    with torch.cuda.device(idx):
        return call(name, *args)


def workspace_layout(n_local, n, d, dtype=F32, flags=0):
    """-> (total_bytes, offsets[WS_NSECTIONS], extra[WSX_N]).  Pure host arithmetic, no GPU needed."""
    total = _sz(0)
    call("stein_workspace_bytes", n_local, n, d, dtype, flags, ctypes.byref(total))
    offs = (_sz * WS_NSECTIONS)()
    extra = (_i64 * WSX_N)()
    call("stein_workspace_layout", n_local, n, d, dtype, flags, offs, extra)
    return int(total.value), [int(o) for o in offs], [int(e) for e in extra]


def layout_folds(n_local, n, d, dtype=F32, flags=0):
    """Does the fused call with these arguments take the folded contraction (FLAG_FOLD)?  Host arithmetic."""
    out = _int(0)
    call("stein_layout_folds", n_local, n, d, dtype, flags, ctypes.byref(out))
    return bool(out.value)


def layout_fold_ranges(n_local, n, d, dtype=F32, flags=0):
    """j ranges of the folded contraction of the fused call with these arguments (0: it does not fold).  Host arithmetic."""
    out = _int(0)
    call("stein_layout_fold_ranges", n_local, n, d, dtype, flags, ctypes.byref(out))
    return int(out.value)


def debug_fold_split(ranges):
    """Test hook (per calling thread): j ranges the folded contraction's plan asks for; 0 restores the plan's own rule."""
    call("stein_debug_fold_split", int(ranges))


def debug_no_warm(off):
    """Test hook (per calling thread): True launches the fused call's select without its warm slice."""
    call("stein_debug_no_warm", 1 if off else 0)


def stream_workspace_bytes(n, d, dtype=F32, flags=0):
    """Workspace bytes of the streaming step (stein_svgd_phi_stream): O(n d), no distance image.  Host arithmetic."""
    total = _sz(0)
    call("stein_stream_workspace_bytes", n, d, dtype, flags, ctypes.byref(total))
    return int(total.value)


def stream_ksd_workspace_bytes(n, d, dtype=F32, flags=0):
    """Workspace bytes of the streaming step with the Stein discrepancy sums (stein_svgd_phi_stream_ksd): the plain step's
    layout with the partial rd and two more sets of block partials behind it.  Host arithmetic."""
    total = _sz(0)
    call("stein_stream_ksd_workspace_bytes", n, d, dtype, flags, ctypes.byref(total))
    return int(total.value)


def stream_plan(n, d):
    """-> (row_tiles, col_groups, jsplit) of the streaming step's grid.  Host arithmetic."""
    rt, cg, js = _int(0), _int(0), _int(0)
    call("stein_stream_plan", n, d, ctypes.byref(rt), ctypes.byref(cg), ctypes.byref(js))
    return int(rt.value), int(cg.value), int(js.value)


def debug_stream_jsplit(jsplit):
    """Test hook (per calling thread): j ranges the streaming step's plan asks for; 0 restores the plan's own rule."""
    call("stein_debug_stream_jsplit", int(jsplit))


def stream_median_workspace_bytes(n, d, dtype=F32, flags=0):
    """Workspace bytes of the streaming median (stein_stream_median): never more than stream_workspace_bytes.  Host arithmetic."""
    total = _sz(0)
    call("stein_stream_median_workspace_bytes", n, d, dtype, flags, ctypes.byref(total))
    return int(total.value)


def stream_median_plan(n, d):
    """-> (byte offset of the [3][2][2048] int64 histograms, byte offset of the 64-byte select state, tiles, workgroups)
    of the streaming median inside its workspace.  Host arithmetic."""
    ho, so, tiles, blocks = _sz(0), _sz(0), _i64(0), _int(0)
    call("stein_stream_median_plan", n, d, ctypes.byref(ho), ctypes.byref(so), ctypes.byref(tiles), ctypes.byref(blocks))
    return int(ho.value), int(so.value), int(tiles.value), int(blocks.value)


def debug_stream_median_grid(blocks):
    """Test hook (per calling thread): workgroups of the streaming median's histogram launches; 0 restores the rule."""
    call("stein_debug_stream_median_grid", int(blocks))


def imq_workspace_bytes(n, d, dtype=F32, flags=0):
    """Workspace bytes of the IMQ step (stein_svgd_phi_imq): O(n d), never less than the streaming median's.  Host arithmetic."""
    total = _sz(0)
    call("stein_imq_workspace_bytes", n, d, dtype, flags, ctypes.byref(total))
    return int(total.value)


def imq_ksd_workspace_bytes(n, d, dtype=F32, flags=0):
    """Workspace bytes of the IMQ step with the Stein discrepancy sums (stein_svgd_phi_imq_ksd): the plain step's layout with
    the partial rd5 and two more sets of block partials behind it.  Host arithmetic."""
    total = _sz(0)
    call("stein_imq_ksd_workspace_bytes", n, d, dtype, flags, ctypes.byref(total))
    return int(total.value)


def imq_plan(n, d):
    """-> (row_tiles, col_blocks, jsplit) of the IMQ step's grid.  Host arithmetic."""
    rt, cb, js = _int(0), _int(0), _int(0)
    call("stein_imq_plan", n, d, ctypes.byref(rt), ctypes.byref(cb), ctypes.byref(js))
    return int(rt.value), int(cb.value), int(js.value)


def thin_workspace_bytes(n, d, dtype=F32, flags=0):
    """Workspace bytes of Stein thinning (stein_thin): O(n), independent of d and of the pick count.  Host arithmetic."""
    total = _sz(0)
    call("stein_thin_workspace_bytes", n, d, dtype, flags, ctypes.byref(total))
    return int(total.value)


def debug_thin_grid(blocks):
    """Test hook (per calling thread): workgroups of Stein thinning's launches (at most 1024); 0 restores the rule."""
    call("stein_debug_thin_grid", int(blocks))


def ksd_boot_workspace_bytes(n, d, reps, dtype=F32, flags=0):
    """Workspace bytes of the KSD test's quadratic forms (stein_ksd_boot): O(n d + n reps).  Host arithmetic."""
    total = _sz(0)
    call("stein_ksd_boot_workspace_bytes", n, d, reps, dtype, flags, ctypes.byref(total))
    return int(total.value)


def ksd_boot_plan(n, d, reps):
    """-> (row_tiles, col_groups, jsplit) of stein_ksd_boot's grid.  Host arithmetic."""
    rt, cg, js = _int(0), _int(0), _int(0)
    call("stein_ksd_boot_plan", n, d, reps, ctypes.byref(rt), ctypes.byref(cg), ctypes.byref(js))
    return int(rt.value), int(cg.value), int(js.value)


def debug_boot_jsplit(jsplit):
    """Test hook (per calling thread): j ranges stein_ksd_boot's plan asks for; 0 restores the plan's own rule."""
    call("stein_debug_boot_jsplit", int(jsplit))


def ksd_matmul_workspace_bytes(n, d, reps, dtype=F32, flags=0):
    """Workspace bytes of the Stein-kernel products (stein_ksd_matmul): O(n d + n reps jsplit).  Host arithmetic."""
    total = _sz(0)
    call("stein_ksd_matmul_workspace_bytes", n, d, reps, dtype, flags, ctypes.byref(total))
    return int(total.value)


def weights_workspace_bytes(n, d, dtype=F32, flags=0):
    """Workspace bytes of the Stein importance weights (stein_weights): O(n d), independent of the iteration count.  Host
    arithmetic."""
    total = _sz(0)
    call("stein_weights_workspace_bytes", n, d, dtype, flags, ctypes.byref(total))
    return int(total.value)


def debug_weights_grid(blocks):
    """Test hook (per calling thread): workgroups of the importance weights' step launches (at most 1024); 0 restores the
    rule.  No bit of the result depends on it."""
    call("stein_debug_weights_grid", int(blocks))


def predict_workspace_bytes(n, batch):
    """Workspace bytes of a stein_predict_* call that asks for a summary (mean, var, lpd): 20 bytes per row and particle
    slice, independent of d.  Host arithmetic."""
    total = _sz(0)
    call("stein_predict_workspace_bytes", n, batch, ctypes.byref(total))
    return int(total.value)


def predict_softmax_workspace_bytes(n, batch, n_classes):
    """Workspace bytes of a stein_predict_softmax call that asks for a summary (prob, lpd, ent, label): 4 (n_classes + 2)
    bytes per row and particle slice, independent of d.  Host arithmetic."""
    total = _sz(0)
    call("stein_predict_softmax_workspace_bytes", n, batch, n_classes, ctypes.byref(total))
    return int(total.value)


def predict_bnn_class_workspace_bytes(n, batch, n_classes):
    """Workspace bytes of a stein_predict_bnn_class call that asks for a summary (prob, lpd, ent, label): 4 (n_classes + 2)
    bytes per row and particle slice, independent of d.  Host arithmetic."""
    total = _sz(0)
    call("stein_predict_bnn_class_workspace_bytes", n, batch, n_classes, ctypes.byref(total))
    return int(total.value)


def predict_softmax_weighted_workspace_bytes(n, batch, n_classes):
    """Workspace bytes of a stein_predict_softmax_weighted call that asks for prob, lpd, ent, label or ess: the unweighted
    size plus the weight pass's per-slice sums.  Host arithmetic."""
    total = _sz(0)
    call("stein_predict_softmax_weighted_workspace_bytes", n, batch, n_classes, ctypes.byref(total))
    return int(total.value)


def predict_bnn_class_weighted_workspace_bytes(n, batch, n_classes):
    """Workspace bytes of a stein_predict_bnn_class_weighted call that asks for prob, lpd, ent, label or ess: the unweighted
    size plus the weight pass's per-slice sums.  Host arithmetic."""
    total = _sz(0)
    call("stein_predict_bnn_class_weighted_workspace_bytes", n, batch, n_classes, ctypes.byref(total))
    return int(total.value)


def debug_score_softmax_lanes(lanes):
    """Test hook (per calling thread): lanes per row of stein_score_softmax's forward phase (a power of two up to 64); 0
    restores the rule.  The order in which a logit's terms are summed follows it."""
    call("stein_debug_score_softmax_lanes", int(lanes))


def predict_weighted_workspace_bytes(n, batch):
    """Workspace bytes of a stein_predict_*_weighted call that asks for mean, var, lpd or ess: the unweighted size plus the
    weight pass's per-slice sums.  Host arithmetic."""
    total = _sz(0)
    call("stein_predict_weighted_workspace_bytes", n, batch, ctypes.byref(total))
    return int(total.value)


def predict_ranks_workspace_bytes(n, batch, n_ranks):
    """Workspace bytes of a stein_predict_*_ranks call: 76 bytes per (row, rank), independent of n and d.  Host arithmetic."""
    total = _sz(0)
    call("stein_predict_ranks_workspace_bytes", n, batch, n_ranks, ctypes.byref(total))
    return int(total.value)


def debug_predict_ranks_slices(slices):
    """Test hook (per calling thread): particle slices of the stein_predict_*_ranks calls (at most 1024); 0 restores the
    plan's own rule.  No bit of the result depends on it."""
    call("stein_debug_predict_ranks_slices", int(slices))


def predict_ranks_weighted_workspace_bytes(n, batch, n_levels):
    """Workspace bytes of a stein_predict_*_ranks_weighted call: 512 bytes and 76 per (row, level), independent of n and d.
    Host arithmetic."""
    total = _sz(0)
    call("stein_predict_ranks_weighted_workspace_bytes", n, batch, n_levels, ctypes.byref(total))
    return int(total.value)


def predict_rank_masses_workspace_bytes(n):
    """Workspace bytes of stein_predict_rank_masses: 24 per workgroup of its grid, at most 6144.  Host arithmetic."""
    total = _sz(0)
    call("stein_predict_rank_masses_workspace_bytes", n, ctypes.byref(total))
    return int(total.value)


def debug_predict_ranks_weighted_bits(bits):
    """Test hook (per calling thread): digit bits per level of the stein_predict_*_ranks_weighted calls (1 .. 4); 0 restores
    the rule.  No bit of the result depends on it."""
    call("stein_debug_predict_ranks_weighted_bits", int(bits))


def predict_ycdf_workspace_bytes(n, batch, n_pts):
    """Workspace bytes of a stein_predict_*_ycdf call: the weight pass's header and n_pts floats per (slice, row), independent
    of d.  Host arithmetic."""
    total = _sz(0)
    call("stein_predict_ycdf_workspace_bytes", n, batch, n_pts, ctypes.byref(total))
    return int(total.value)


def predict_yquantiles_workspace_bytes(n, batch, n_levels):
    """Workspace bytes of a stein_predict_*_yquantiles call: the weight pass's header, two floats per (row, level) and
    7 n_levels floats per (slice, row), independent of d.  Host arithmetic."""
    total = _sz(0)
    call("stein_predict_yquantiles_workspace_bytes", n, batch, n_levels, ctypes.byref(total))
    return int(total.value)


def version():
    return load().stein_version()


def timing_reserve(calls):
    """Reserve HIP events for `calls` fused calls made with FLAG_TIMING (and rewind the cursor)."""
    call("stein_timing_reserve", int(calls))


def timing_read(max_calls):
    """-> list of {stage: ms} for the timed fused calls since timing_reserve (waits for their events)."""
    buf = (_c.c_float * (max_calls * len(T_STAGES)))()
    got = _int(0)
    call("stein_timing_read", buf, int(max_calls), _c.byref(got))
    k = len(T_STAGES)
    return [{T_STAGES[j]: float(buf[i * k + j]) for j in range(k)} for i in range(got.value)]
