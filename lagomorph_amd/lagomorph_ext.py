"""``lagomorph_ext`` for MI355X: the reference's 13-function extension surface
(``/root/reference/lagomorph/extension/extension.cpp:175-189``) bound with
ctypes onto ``liblagomorph_hip.so`` (C ABI in ``include/lagomorph_hip.h``).

Same names, argument order, defaults and return conventions as the pybind11
module the reference builds with ``CUDAExtension`` (``setup.py:18-31``):
inputs are borrowed contiguous device tensors, outputs are freshly allocated
tensors, ``fluid_operator`` mutates its first argument, argument violations
raise ``RuntimeError`` (the reference's ``TORCH_CHECK``).  Kernels are launched
on torch's *current* HIP stream (the reference used the legacy default stream).

There is no CPU path: every entry point raises on a CPU tensor, and importing
this module raises if the HIP library has not been built
(``python -m lagomorph_amd.build`` / ``__graft_entry__.build()``).
"""
import ctypes
import math
import threading
import os

import torch  # must be imported first: it loads the process's libamdhip64.so.7

_HERE = os.path.dirname(os.path.abspath(__file__))
# LAGO_HIP_LIBRARY selects another build of the same C ABI (tools/ use the -DLAGO_PROFILING build this way)
LIB_PATH = os.environ.get("LAGO_HIP_LIBRARY") or os.path.join(_HERE, "_lib", "liblagomorph_hip.so")
ABI_VERSION = 5  # LAGO_ABI_VERSION of include/lagomorph_hip.h this binding was written against

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: the HIP extension is not built "
        "(run `python -m lagomorph_amd.build`); lagomorph_amd has no CPU fallback"
    )
_lib = ctypes.CDLL(LIB_PATH)
_lib.lago_abi_version.restype = ctypes.c_int
if _lib.lago_abi_version() != ABI_VERSION:
    # a stale library would be called with shifted arguments (memory corruption, not an error): refuse it
    raise ImportError(
        f"{LIB_PATH} has C-ABI version {_lib.lago_abi_version()}, this binding needs {ABI_VERSION}: "
        "rebuild it with `python -m lagomorph_amd.build -f`"
    )
_lib.lago_last_error.restype = ctypes.c_char_p
_lib.lago_version.restype = ctypes.c_char_p

_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_dbl = ctypes.c_double

# argtypes per entry point (both precisions) -- mirrors include/lagomorph_hip.h
_SIGS = {
    "lago_interp_forward": [_vp, _vp, _vp, _dbl, _int, _i64, _i64, _i64, _i64, _i64, _int, _vp],
    "lago_interp_backward": [_vp, _vp, _vp, _vp, _vp, _dbl, _int, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _vp],
    "lago_interp_hessian_diagonal_image": [_vp, _vp, _dbl, _i64, _i64, _i64, _i64, _i64, _vp],
    "lago_jtv_forward": [_vp, _vp, _vp, _int, _int, _int, _i64, _i64, _i64, _i64, _i64, _vp],
    "lago_jtv_backward": [_vp, _vp, _vp, _vp, _vp, _int, _int, _int, _i64, _i64, _i64, _i64, _i64, _vp],
    "lago_jtv_adjoint_forward": [_vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _vp],
    "lago_jtv_adjoint_backward": [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_fluid_operator": [_vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _dbl, _dbl, _dbl, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_affine_interp_forward": [_vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _int, _vp],
    "lago_affine_interp_backward": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _int, _int,
                                    _int, _int, _vp],
    "lago_regrid_forward": [_vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp],
    "lago_regrid_backward_sep": [_vp, _vp, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp],
    "lago_regrid_backward": [_vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp],
    "lago_compose": [_vp, _vp, _vp, _dbl, _dbl, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_compose_near": [_vp, _vp, _vp, _dbl, _dbl, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_lincomb": [_vp, _int, _vp, _vp, _vp, _vp, _dbl, _dbl, _dbl, _dbl, _i64, _vp],
    "lago_Ad_star": [_vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_interp_backward_fused": [_vp, _vp, _vp, _vp, _vp, _dbl, _int, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _int,
                                   _dbl, _vp],
    "lago_jtv_backward_acc": [_vp, _vp, _vp, _vp, _vp, _int, _int, _int, _i64, _i64, _i64, _i64, _i64, _int, _vp],
    "lago_ad_star": [_vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_jacdet_forward": [_vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_jacdet_backward": [_vp, _vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_invert_disp_forward": [_vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_invert_disp_adjoint": [_vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_gauss_smooth": [_vp, _vp, _vp, _vp, _vp, _int, _dbl, _int, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_lncc_moments": [_vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_lncc_cc": [_vp, _vp, _dbl, _i64, _vp],
    "lago_lncc_coeffs": [_vp, _vp, _vp, _dbl, _int, _i64, _vp],
    "lago_lncc_combine": [_vp, _vp, _vp, _vp, _vp, _int, _i64, _vp],
    "lago_mi_histogram": [_vp, _vp, _vp, _vp, _i64, _int, _dbl, _dbl, _dbl, _dbl, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_mi_backward": [_vp, _vp, _vp, _vp, _vp, _int, _dbl, _dbl, _dbl, _dbl, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_warp_labels": [_vp, _vp, _vp, _dbl, _int, _int, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_interp_points": [_vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _int, _vp],
    "lago_interp_points_backward": [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _vp],
    "lago_bspline_prefilter": [_vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _vp],
    "lago_interp_bspline": [_vp, _vp, _vp, _dbl, _int, _i64, _i64, _i64, _i64, _i64, _int, _vp],
    "lago_interp_bspline_backward": [_vp, _vp, _vp, _vp, _vp, _dbl, _int, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _vp],
    "lago_ffd_expand": [_vp, _vp, _int, _i64, _i64, _i64, _i64, _int, _int, _int, _vp],
    "lago_ffd_expand_adjoint": [_vp, _vp, _vp, _i64, _int, _i64, _i64, _i64, _i64, _int, _int, _int, _vp],
    "lago_field_energy": [_vp, _vp, _vp, _i64, _int, _int, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_dbl), _vp],
    "lago_field_energy_operator": [_vp, _vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_dbl), _vp],
    "lago_pyramid_down": [_vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _dbl, _vp],
    "lago_pyramid_up": [_vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _dbl, _vp],
    "lago_fluid_metric": [_vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _dbl, _dbl, _dbl, _int, _i64, _i64,
                          _i64, _i64, _vp],
    "lago_fluid_metric_scaled": [_vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _dbl, _dbl, _dbl, _int, _i64,
                                 _i64, _i64, _i64, _dbl, _vp],
}


class LagoTuning(ctypes.Structure):
    """include/lagomorph_hip.h: lago_tuning (field order and types as declared there)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("splat_mode", ctypes.c_int32), ("splat_tile", ctypes.c_int32 * 7),
                ("splat_shear", ctypes.c_int32 * 8), ("splat_shear_mc", ctypes.c_int32), ("splat_mc", ctypes.c_int32),
                ("vector_kernels", ctypes.c_int32), ("launch_order", ctypes.c_int32), ("stencil_tile", ctypes.c_int32),
                ("gather_window", ctypes.c_int32), ("fluid_mode", ctypes.c_int32), ("fluid_xpass_ipw", ctypes.c_int32),
                ("fluid_zy_persist", ctypes.c_int32), ("fluid_xpass_wide", ctypes.c_int32),
                ("fluid_xpass_persist", ctypes.c_int32), ("affine_box", ctypes.c_int32), ("compose_near", ctypes.c_int32)]


# (argtypes, restype) of the symbols without a precision suffix: scratch queries, the integer-label kernels, counters, tuning
_PLAIN_SIGS = {
    "lago_set_debug": ([_int], _int),
    "lago_mi_scratch_tables": ([_int, _i64, _i64], _int),
    "lago_label_overlap": ([_vp, _vp, _vp, _vp, _i64, _int, _i64, _i64, _vp], _int),
    "lago_label_overlap_scratch_chunks": ([_int, _i64, _i64], _int),
    "lago_distance_transform": ([_vp, _vp, _int, ctypes.c_int32, ctypes.POINTER(_dbl), _int, _int, _i64, _i64, _i64, _i64,
                                 _vp], _int),
    "lago_ffd_scratch_elems": ([_int, _i64, _i64, _i64, _i64, _int, _int, _int], ctypes.c_longlong),
    "lago_field_energy_scratch_elems": ([_int, _int, _i64, _i64, _i64, _i64, _i64], ctypes.c_longlong),
    "lago_get_tuning": ([ctypes.POINTER(LagoTuning)], None),
    "lago_default_tuning": ([ctypes.POINTER(LagoTuning)], None),
    "lago_set_tuning": ([ctypes.POINTER(LagoTuning)], _int),
    "lago_path_launches": ([_int], ctypes.c_longlong),
    "lago_reversed_launches": ([], ctypes.c_longlong),
}
_fn = {}   # the typed entry points _call dispatches on; the unsuffixed symbols are reached as _lib.<name>
for _name, _args in _SIGS.items():
    for _suf in ("_f32", "_f64"):
        _f = getattr(_lib, _name + _suf, None)
        if _f is None:
            continue
        _f.argtypes, _f.restype = _args, _int
        _fn[_name + _suf] = _f
for _name, (_args, _res) in _PLAIN_SIGS.items():
    _f = getattr(_lib, _name)   # a library without one of these fails here, at import
    _f.argtypes, _f.restype = _args, _res
_tune_lock = threading.Lock()


def _tuning_struct(getter):
    t = LagoTuning()
    t.struct_size = ctypes.sizeof(LagoTuning)
    getter(ctypes.byref(t))
    return t


def _as_dict(t):
    return {n: (list(getattr(t, n)) if hasattr(getattr(t, n), "__len__") else int(getattr(t, n)))
            for n, _ in LagoTuning._fields_ if n != "struct_size"}


def get_tuning():
    """The tuning settings in force (include/lagomorph_hip.h: lago_tuning) as a dict."""
    return _as_dict(_tuning_struct(_lib.lago_get_tuning))


def default_tuning():
    return _as_dict(_tuning_struct(_lib.lago_default_tuning))


def tune(**fields):
    """Change some tuning settings (process-wide, speed only): read the struct, replace the named fields, write it back.
    tune(splat_shear_mc=1), tune(splat_shear=[1, 8, 6, 0, 1, 1, 4, 1024]), ...; tune(**default_tuning()) restores all."""
    with _tune_lock:
        t = _tuning_struct(_lib.lago_get_tuning)
        for k, v in fields.items():
            if k == "struct_size" or k not in dict(LagoTuning._fields_):
                raise KeyError(f"lago_tuning has no field {k!r}")
            cur = getattr(t, k)
            if hasattr(cur, "__len__"):
                v = [int(x) for x in v]
                if len(v) != len(cur):
                    raise ValueError(f"lago_tuning.{k} takes {len(cur)} values")
                for i, x in enumerate(v):
                    cur[i] = x
            else:
                setattr(t, k, int(v))
        if _lib.lago_set_tuning(ctypes.byref(t)) != 0:
            raise RuntimeError(_lib.lago_last_error().decode())


def _suffix(t):
    if t.dtype == torch.float32:
        return "_f32"
    if t.dtype == torch.float64:
        return "_f64"
    raise RuntimeError(f"lagomorph_ext: only float32 and float64 are supported (got {t.dtype})")


# ---------------------------------------------------------------------------
# The argument frame: one function per decision an entry point takes before its launch.  An entry point is a sequence
# of these calls, and the order of its calls is the order in which it reports errors.  Two orders are in use:
#   device first  the reference's surface (interp, jtv, affine, regrid, fluid_operator) and the fused kernels beside
#                 it (compose, lincomb, Ad_star, ad_star, mi): _check_input on each tensor, as the reference's
#                 CHECK_INPUT did, then _same -- through _check_inputs, or written out where one tensor is checked,
#                 something stands between the two steps (mi, lincomb) or the call is timed as launch latency
#                 (interp, affine)
#   device last   the newer families (gauss, lncc, invert, labels, edt, points, bspline, ffd, energy): _check_types,
#                 the family's shape checks, then _check_layout or _check_cuda, so that every other error shows on a
#                 CPU tensor too
# Nothing here reads a tensor's values: shapes, dtypes, devices, strides and data_ptr() only.


def _check_tensors(named):
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")


def _check_input(x, name):
    # CHECK_INPUT, extension.cpp:8-10 (on the path of every call: the type check is written out, not a _check_tensors call)
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not x.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not x.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _same(ref, *others):
    for o in others:
        if o.dtype != ref.dtype:
            raise RuntimeError(f"lagomorph_ext: dtype mismatch ({ref.dtype} vs {o.dtype})")
        if o.device != ref.device:
            raise RuntimeError(f"lagomorph_ext: device mismatch ({ref.device} vs {o.device})")


def _check_inputs(named):
    """Device first: every (name, tensor) pair passes CHECK_INPUT, then all share the first one's dtype and device."""
    for name, t in named:
        _check_input(t, name)
    _same(named[0][1], *[t for _, t in named[1:]])


def _check_types(named):
    """Every (name, tensor) pair is a tensor of one supported floating dtype, the first one's."""
    _check_tensors(named)
    for name, t in named:
        _suffix(t)
    for name, t in named[1:]:
        if t.dtype != named[0][1].dtype:
            raise RuntimeError(f"lagomorph_ext: dtype mismatch ({named[0][1].dtype} vs {t.dtype})")


def _check_layout(named):
    """Contiguity, then -- last, so that every other error is raised whatever device the tensors are on -- the devices."""
    for name, t in named:
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")
    for name, t in named[1:]:
        if t.device != named[0][1].device:
            raise RuntimeError(f"lagomorph_ext: device mismatch ({named[0][1].device} vs {t.device})")
    for name, t in named:
        _check_input(t, name)


def _check_cuda(named):
    """The device check of the entry points that make their inputs contiguous themselves."""
    for name, t in named:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")


def _spatial(t):
    d = t.dim() - 2
    if d == 2:
        return 2, t.size(2), t.size(3), 1
    if d == 3:
        return 3, t.size(2), t.size(3), t.size(4)
    return d, 0, 0, 0


def _spatial_frame(t, message):
    """(dim, nx, ny, nz) of a channel-first tensor (N, C, *sp) as the C side takes them: the family's error unless it has
    two or three spatial axes."""
    frame = _spatial(t)
    if frame[0] not in (2, 3):
        raise RuntimeError(message)
    return frame


def _pad(values, fill, n=3):
    """Per-axis values (extents, spacings, origins, LUT pointers) as the n arguments the C call takes, unused axes as `fill`."""
    values = tuple(values)
    return values + (fill,) * (n - len(values))


def _broadcast(field, nn, message, empty=False):
    """Is `field`, of nn items or of one, broadcast over a batch of nn?  RuntimeError(message) for any other pair of batch
    sizes.  One item against an empty batch is an error on the reference's surface and passes with `empty` (the newer
    families, which accept a batch size in (1, nn))."""
    n = field.size(0)
    if n != nn and (n != 1 or (nn == 0 and not empty)):
        raise RuntimeError(message)
    return n < nn


def _on_grid(u, I, dim):
    """Is u a vector field on I's grid: `dim` channels and I's spatial shape?"""
    return u.size(1) == dim and tuple(u.shape[2:]) == tuple(I.shape[2:])


def _overlaps(a, b):
    """Do the byte ranges of two contiguous tensors intersect?  (a partially overlapping view counts: the kernel
    gathers from its inputs while it writes `out`)"""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a.numel() > 0 and b.numel() > 0 and a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _check_dest(out, name, ref, message, *inputs):
    """A caller-supplied destination: a contiguous device tensor of ref's dtype and device, then RuntimeError(message)
    unless it has ref's shape and its bytes overlap none of `inputs`."""
    _check_input(out, name)
    _same(ref, out)
    if out.shape != ref.shape or any(_overlaps(out, x) for x in inputs):
        raise RuntimeError(message)


def _scratch_elems(query, *args):
    """The scratch size a `*_scratch_elems` query of the library gives; its error when the arguments do not fit."""
    elems = int(query(*args))
    if elems < 0:
        raise RuntimeError(_lib.lago_last_error().decode("utf-8", "replace"))
    return elems


def _env_flag(name):
    """A profiling variable of the environment: None when unset, else whether it is switched on (parsed defensively: an
    empty or odd value must not break `import lagomorph_amd`)."""
    v = os.environ.get(name)
    return None if v is None else v.strip().lower() not in ("", "0", "off", "false", "no")


def _call(name, ref, *args):
    """Launch on torch's current stream of ref's device; raise RuntimeError on failure."""
    _launch(_fn[name + _suffix(ref)], ref, *args)


def _launch(f, ref, *args):
    if ref.device.index != torch.cuda.current_device():
        with torch.cuda.device(ref.device):
            rc = f(*args, torch.cuda.current_stream().cuda_stream)
    else:
        rc = f(*args, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(_lib.lago_last_error().decode("utf-8", "replace"))


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() > 0 else None


# ---------------------------------------------------------------------------


def set_debug_mode(mode):
    """extension.cpp:105-107.  In debug mode every launch is followed by a
    stream synchronise and kernel faults raise (the reference printed them)."""
    _lib.lago_set_debug(1 if mode else 0)


def set_splat_mode(mode):
    """0 = global atomics only, 1 = LDS-privatised splat (default)."""
    tune(splat_mode=mode)


def set_splat_tile(tx, ty, tz, mx, my, mz, nthreads):
    tune(splat_tile=[tx, ty, tz, mx, my, mz, nthreads])


def set_splat_shear(on=1, tx=8, ty=6, tz=0, mx=1, my=1, mz=4, nthreads=1024):
    """Sheared-window float32 splat (csrc/splat.hip: splat_shear_kernel): on/off and its tile.  Speed only."""
    tune(splat_shear=[on, tx, ty, tz, mx, my, mz, nthreads])


def set_splat_mc(on):
    """General tiled splat: 1 (default) the multi-channel single-pass form where it applies.  Speed only."""
    tune(splat_mc=1 if on else 0)


def set_splat_shear_mc(mode):
    """Sheared-window splat, several channels with d_u: 2 (default) geometry and d_u sums in registers over the
    channels, 1 the d_u sums only, 0 neither.  Speed only (same d_u bits)."""
    tune(splat_shear_mc=mode)


def set_fluid_tuning(xpass_ipw=0, zy_persist=1, xpass_wide=1, xpass_persist=1):
    """FFT-pass fluid metric: batch items per x-pass workgroup (0 = by launch size), persistent zy kernels for
    planes above 80 KB, 512-thread x pass for the 256-point tile, persistent prefetching x-pass grid.  Speed only."""
    tune(fluid_xpass_persist=xpass_persist, fluid_xpass_ipw=xpass_ipw, fluid_zy_persist=1 if zy_persist else 0,
         fluid_xpass_wide=1 if xpass_wide else 0)


def set_launch_order(alternate):
    """1 (default): successive launches walk their workgroups in alternating directions (a consumer starts on what
    its producer wrote last: Infinity-Cache reuse); 0: always ascending.  Speed only."""
    tune(launch_order=1 if alternate else 0)


def set_stencil_tile(on):
    """1 (default): LDS row-tile stencil kernels (Ad_star, jacobian_times_vectorfield_backward) where shapes allow;
    0: the direct one-lane-per-voxel kernels; 3: row tiles without the compile-time-geometry instantiations for 128^3 /
    160^3 volumes.  Same bits."""
    tune(stencil_tile=on)


PATHS = ("gather_window", "stencil_tile", "vector_gather", "splat_shear", "splat_shear_mc", "splat_tiled", "splat_global",
         "fluid_lds", "fluid_2d", "fluid_xpass", "fluid_rocfft", "splat_2d", "splat_affine_box", "fluid_generic",
         "gather_window_near")  # LAGO_PATH_* of include/lagomorph_hip.h, in order


def reversed_launches():
    """Launches so far that walked their workgroups in descending order (include/lagomorph_hip.h)."""
    return int(_lib.lago_reversed_launches())


def path_launches(name=None):
    """Launches so far per implementation path (a dict), or of one path by name."""
    if name is not None:
        return int(_lib.lago_path_launches(PATHS.index(name)))
    return {p: int(_lib.lago_path_launches(i)) for i, p in enumerate(PATHS)}


def set_gather_window(on):
    """1 (default): float32 3D gathers through an LDS window (compose) where shapes allow; 0: pair gathers
    through the vector L1 only.  Same bits."""
    tune(gather_window=1 if on else 0)


def set_compose_near(on):
    """1 (default): `compose(..., near_identity=True)` takes the fixed-origin LDS-window kernel with two windows in flight
    where the shape allows the window kernels; 0: the hint is ignored.  Same bits."""
    tune(compose_near=1 if on else 0)


if _env_flag("LAGO_GATHER_WINDOW") is not None:  # profiling convenience: A/B under rocprofv3 without code changes
    set_gather_window(_env_flag("LAGO_GATHER_WINDOW"))


if _env_flag("LAGO_COMPOSE_NEAR") is not None:  # the same convenience for the near-identity arm of compose
    set_compose_near(_env_flag("LAGO_COMPOSE_NEAR"))


def set_vector_kernels(on):
    """1 (default): slab-unrolled 3D gather kernels (two voxels per lane) where shapes allow; 0: one-voxel-per-lane kernels only."""
    tune(vector_kernels=1 if on else 0)


def set_fluid_mode(mode):
    """fluid_metric implementation: 3 (default) the tuned LDS-tiled FFT passes where the shape allows and the generic
    hand-written passes for everything else (no rocFFT); 2 the tuned passes with rocFFT fallbacks, 1 rocFFT 2D plan +
    fused x pass, 0 rocFFT 3D plan + operator kernel; 4 = 3 with the generic passes' x transforms and operator as three
    launches instead of the fused one (same bits: the comparison switch of that fusion)."""
    tune(fluid_mode=mode)


def version():
    return _lib.lago_version().decode()


def interp_forward(Iv, u, dt=1.0):
    """extension.cpp:135-143 -> cuda/interp.cu:80-130"""
    _check_input(Iv, "Iv")
    _check_input(u, "u")
    _same(Iv, u)
    dim, nx, ny, nz = _spatial_frame(Iv, "Only two- and three-dimensional interpolation is supported")
    if u.dim() != Iv.dim() or not _on_grid(u, Iv, dim):
        raise RuntimeError(f"interp_forward: displacement of shape {tuple(u.shape)} does not match image {tuple(Iv.shape)}")
    nn = u.size(0)
    bc = _broadcast(Iv, nn, "interp_forward: batch sizes of I and u are incompatible")
    out = torch.empty((nn, Iv.size(1)) + tuple(Iv.shape[2:]), dtype=Iv.dtype, device=Iv.device)
    _call("lago_interp_forward", Iv, _ptr(out), _ptr(Iv), _ptr(u), float(dt), dim, nn, Iv.size(1), nx, ny, nz, int(bc))
    return out


def _interp_backward_args(grad_out, I, u):
    """The argument block interp_backward and interp_backward_fused share: (dim, nx, ny, nz, nn, broadcast)."""
    _check_input(grad_out, "grad_out")
    _check_input(I, "I")
    _check_input(u, "u")
    _same(I, u, grad_out)
    dim, nx, ny, nz = _spatial_frame(I, "Only two- and three-dimensional interpolation is supported")
    nn = u.size(0)
    bc = _broadcast(I, nn, "interp_backward: batch sizes of I and u are incompatible")
    if tuple(grad_out.shape) != (nn, I.size(1)) + tuple(I.shape[2:]) or u.dim() != I.dim() or not _on_grid(u, I, dim):
        raise RuntimeError("interp_backward: grad_out / I / u shapes are inconsistent")
    return dim, nx, ny, nz, nn, bc


def interp_backward(grad_out, I, u, dt, need_I, need_u):
    """extension.cpp:145-156 -> cuda/interp.cu:246-313.  Returns [d_I, d_u]; both always allocated."""
    dim, nx, ny, nz, nn, bc = _interp_backward_args(grad_out, I, u)
    d_I = torch.empty_like(I)
    d_u = torch.empty_like(u)
    _call("lago_interp_backward", I, _ptr(d_I), _ptr(d_u), _ptr(grad_out), _ptr(I), _ptr(u), float(dt), dim, nn,
          I.size(1), nx, ny, nz, int(bc), int(bool(need_I)), int(bool(need_u)))
    return [d_I, d_u]


def interp_hessian_diagonal_image(Iv, u, dt):
    """cuda/interp.cu:351-381 (2D only; accumulates into plane 0 like the reference)."""
    _check_inputs((("Iv", Iv), ("u", u)))
    if Iv.dim() != 4 or u.dim() != 4 or u.size(1) != 2:
        raise RuntimeError("interp_hessian_diagonal_image is only implemented for two-dimensional images")
    nn = max(u.size(0), Iv.size(0))
    out = torch.empty_like(Iv)
    _call("lago_interp_hessian_diagonal_image", Iv, _ptr(out), _ptr(u), float(dt), Iv.size(0), nn, Iv.size(1),
          Iv.size(2), Iv.size(3))
    return out


_JTV_DIMS = "Only two- and three-dimensional jacobian times vectorfield is supported"


def _check_jtv(g, v):
    """A pair of the jtv family, which makes its inputs contiguous itself (the second of any pair reports as "v")."""
    _check_cuda((("g", g), ("v", v)))
    _same(g, v)


def jacobian_times_vectorfield_forward(g, v, displacement, transpose):
    """cuda/diff.cu:129-185: (Dg + [displacement] I) v, or its transpose."""
    _check_jtv(g, v)
    g, v = g.contiguous(), v.contiguous()
    dim, nx, ny, nz = _spatial_frame(g, _JTV_DIMS)
    if g.size(0) != v.size(0):
        raise RuntimeError("arguments must have same batch size dimension")
    if not _on_grid(v, g, dim):
        raise RuntimeError("vector field is of wrong dimension")
    out = torch.empty_like(g)
    _call("lago_jtv_forward", g, _ptr(out), _ptr(g), _ptr(v), int(bool(displacement)), int(bool(transpose)), dim,
          g.size(0), g.size(1), nx, ny, nz)
    return out


def jacobian_times_vectorfield_backward(grad_out, v, w, displacement, transpose, need_v, need_w, d_v=None):
    """cuda/diff.cu:475-540 (need_v / need_w are ignored there: both gradients are always computed).  Beyond the
    reference: with `d_v` given, the gradient is added onto it in place (lago_jtv_backward_acc)."""
    _check_jtv(v, w)
    _check_jtv(v, grad_out)
    grad_out, v, w = grad_out.contiguous(), v.contiguous(), w.contiguous()
    dim, nx, ny, nz = _spatial_frame(v, _JTV_DIMS)
    if v.size(0) != w.size(0):
        raise RuntimeError("arguments must have same batch size dimension")
    if not _on_grid(w, v, dim) or grad_out.shape != v.shape:
        raise RuntimeError("vector field is of wrong dimension")
    d_w = torch.empty_like(w)
    if d_v is not None:
        _check_dest(d_v, "d_v", v, "jacobian_times_vectorfield_backward: d_v must have the shape of v")
        _call("lago_jtv_backward_acc", v, _ptr(d_v), _ptr(d_w), _ptr(grad_out), _ptr(v), _ptr(w), int(bool(displacement)),
              int(bool(transpose)), dim, v.size(0), v.size(1), nx, ny, nz, 1)
        return [d_v, d_w]
    d_v = torch.empty_like(v)
    _call("lago_jtv_backward", v, _ptr(d_v), _ptr(d_w), _ptr(grad_out), _ptr(v), _ptr(w), int(bool(displacement)),
          int(bool(transpose)), dim, v.size(0), v.size(1), nx, ny, nz)
    return [d_v, d_w]


def jacobian_times_vectorfield_adjoint_forward(g, v):
    """cuda/diff.cu:634-672"""
    _check_jtv(g, v)
    g, v = g.contiguous(), v.contiguous()
    dim, nx, ny, nz = _spatial_frame(g, _JTV_DIMS)
    if not _on_grid(v, g, dim) or v.size(0) != g.size(0):
        raise RuntimeError("vector field is of wrong dimension")
    out = torch.empty_like(g)
    _call("lago_jtv_adjoint_forward", g, _ptr(out), _ptr(g), _ptr(v), dim, g.size(0), g.size(1), nx, ny, nz)
    return out


def jacobian_times_vectorfield_adjoint_backward(grad_out, v, w, need_v, need_w):
    """cuda/diff.cu:783-835"""
    _check_jtv(v, w)
    _check_jtv(v, grad_out)
    grad_out, v, w = grad_out.contiguous(), v.contiguous(), w.contiguous()
    dim, nx, ny, nz = _spatial_frame(v, _JTV_DIMS)
    if w.size(1) != dim or v.size(1) != dim or v.shape != w.shape or grad_out.shape != v.shape:
        raise RuntimeError("vector field is of wrong dimension")
    d_v, d_w = torch.empty_like(v), torch.empty_like(w)
    _call("lago_jtv_adjoint_backward", v, _ptr(d_v), _ptr(d_w), _ptr(grad_out), _ptr(v), _ptr(w), dim, v.size(0), nx,
          ny, nz)
    return [d_v, d_w]


def _check_jacdet(u):
    _check_cuda((("u", u),))
    _suffix(u)
    dim, nx, ny, nz = _spatial_frame(u, "Only two- and three-dimensional jacobian determinant is supported")
    if u.size(1) != dim:
        raise RuntimeError("jacobian determinant is only defined for vector fields")
    return dim, nx, ny, nz


def jacobian_determinant_forward(u, displacement):
    """det(Du + [displacement] I) with the clamped central differences of jacobian_times_vectorfield_forward, as an
    image (N, 1, *sp).  Not in the reference (csrc/diff.hip: jacdet_fwd_kernel)."""
    dim, nx, ny, nz = _check_jacdet(u)
    u = u.contiguous()
    out = torch.empty((u.size(0), 1) + tuple(u.shape[2:]), dtype=u.dtype, device=u.device)
    _call("lago_jacdet_forward", u, _ptr(out), _ptr(u), int(bool(displacement)), dim, u.size(0), nx, ny, nz)
    return out


def jacobian_determinant_backward(grad_out, u, displacement):
    """d_u of jacobian_determinant_forward for grad_out of shape (N, 1, *sp): one gather pass, no atomics
    (csrc/diff.hip: jacdet_bwd_kernel)."""
    dim, nx, ny, nz = _check_jacdet(u)
    _check_jtv(u, grad_out)
    if tuple(grad_out.shape) != (u.size(0), 1) + tuple(u.shape[2:]):
        raise RuntimeError("jacobian_determinant_backward: grad_out must have shape (N, 1, *spatial)")
    grad_out, u = grad_out.contiguous(), u.contiguous()
    d_u = torch.empty_like(u)
    _call("lago_jacdet_backward", u, _ptr(d_u), _ptr(grad_out), _ptr(u), int(bool(displacement)), dim, u.size(0), nx,
          ny, nz)
    return d_u


def _check_invert(u, name="u"):
    _check_types(((name, u),))
    dim, nx, ny, nz = _spatial_frame(u, "Only two- and three-dimensional displacement inversion is supported")
    if u.size(1) != dim:
        raise RuntimeError(f"invert_displacement: {name} must be a vector field (N, d, *spatial) with d = len(spatial), "
                           f"got {tuple(u.shape)}")
    _check_cuda(((name, u),))
    return dim, nx, ny, nz


def invert_displacement_forward(u, iters):
    """`iters` steps of v_0 = -u, v_{k+1}(x) = -u(x + v_k(x)) in one kernel (csrc/invert.hip: invert_disp_kernel); the
    bits of `v = -u; for k in range(iters): v = -interp_forward(u, v, 1.0)`.  Not in the reference."""
    iters = int(iters)
    if iters < 0:
        raise RuntimeError(f"invert_displacement: iters must not be negative (got {iters})")
    dim, nx, ny, nz = _check_invert(u)
    u = u.contiguous()
    out = torch.empty_like(u)
    _call("lago_invert_disp_forward", u, _ptr(out), _ptr(u), iters, dim, u.size(0), nx, ny, nz)
    return out


def invert_displacement_adjoint(grad_out, u, v):
    """lam = -(I + (Du)(x + v))^-T grad_out per voxel (csrc/invert.hip: invert_disp_adjoint_kernel): the adjoint solve of
    the converged inverse v of u; d_u is interp_backward(lam, u, v, 1.0, True, False)[0].  One gather pass, no atomics."""
    dim, nx, ny, nz = _check_invert(u)
    for x, nm in ((grad_out, "grad_out"), (v, "v")):
        _check_invert(x, nm)
        if x.shape != u.shape:
            raise RuntimeError(f"invert_displacement_adjoint: {nm} must have the shape of u")
    _same(u, grad_out, v)
    grad_out, u, v = grad_out.contiguous(), u.contiguous(), v.contiguous()
    lam = torch.empty_like(u)
    _call("lago_invert_disp_adjoint", u, _ptr(lam), _ptr(grad_out), _ptr(u), _ptr(v), dim, u.size(0), nx, ny, nz)
    return lam


GAUSS_MAX_RADIUS = 32   # LAGO_GAUSS_MAX_RADIUS of include/lagomorph_hip.h
GAUSS_MODES = {"wrap": 0, "zero": 1}   # LAGO_GAUSS_WRAP / LAGO_GAUSS_ZERO
_GAUSS_DIMS = "Only two- and three-dimensional gaussian smoothing is supported"   # smooth._plan raises it too


def gaussian_smooth_forward(x, radii, taps, mode, alpha=1.0, out=None, accumulate=False):
    """alpha * G x (+ out when accumulate): separable filtering of x (N, C, *sp) with symmetric taps, one kernel per
    axis with a radius > 0 (csrc/gauss.hip).  radii: one int per spatial axis; taps: per axis the 2 r + 1 float64 taps
    (ignored where r == 0); mode "wrap" or "zero".  The result is `out` when given (like x, not overlapping it), a new
    tensor otherwise.  One scratch tensor like x is allocated here when two or more axes are filtered.  Not in the
    reference; no CPU path."""
    _check_types((("x", x),))
    dim, nx, ny, nz = _spatial_frame(x, _GAUSS_DIMS)
    radii, half = _gauss_half_taps("gaussian_smooth", dim, radii, taps, mode)
    if accumulate and out is None:
        raise RuntimeError("gaussian_smooth: accumulate needs out")
    _check_cuda((("x", x),))
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    else:
        _check_dest(out, "out", x, "gaussian_smooth: out must have the shape of x")
        if _overlaps(out, x):
            raise RuntimeError("gaussian_smooth: out must not overlap x")
    scratch = torch.empty_like(x) if sum(r > 0 for r in radii) >= 2 else None
    rad = (ctypes.c_int * dim)(*radii)
    whole = 64 if x.dtype == torch.float32 else 32
    if accumulate and sum(r > 0 for r in radii) == 3 and nz > 1024 and nx > whole and ny > whole:
        # the one shape class whose three-pass accumulate form has no in-place middle pass (include/lagomorph_hip.h):
        # the sum is taken here instead, from alpha * G x in a tensor of its own
        term = torch.empty_like(x)
        _call("lago_gauss_smooth", x, _ptr(term), _ptr(x), _ptr(scratch), rad, half, GAUSS_MODES[mode], float(alpha), 0,
              dim, x.size(0) * x.size(1), nx, ny, nz)
        return out.add_(term)
    _call("lago_gauss_smooth", x, _ptr(out), _ptr(x), _ptr(scratch), rad, half, GAUSS_MODES[mode], float(alpha),
          int(bool(accumulate)), dim, x.size(0) * x.size(1), nx, ny, nz)
    return out


def _gauss_mode(what, mode):
    if mode not in GAUSS_MODES:
        raise ValueError(f"{what}: unknown mode {mode!r} (one of {sorted(GAUSS_MODES)})")
    return GAUSS_MODES[mode]


def _gauss_half_taps(what, dim, radii, taps, mode):
    """The mode / radius / tap checks of the entry point `what`: (radii as ints, the half-tap block lago_gauss_smooth takes)."""
    _gauss_mode(what, mode)
    radii = [int(r) for r in radii]
    if len(radii) != dim or len(taps) != dim:
        raise ValueError(f"{what}: {dim} radii and tap vectors are needed, one per spatial axis")
    half = (ctypes.c_double * (dim * (GAUSS_MAX_RADIUS + 1)))()
    for a, r in enumerate(radii):
        if r < 0 or r > GAUSS_MAX_RADIUS:
            raise ValueError(f"{what}: radius {r} on axis {a} is outside 0..{GAUSS_MAX_RADIUS}")
        if r > 0:
            t = [float(v) for v in taps[a]]
            if len(t) != 2 * r + 1:
                raise ValueError(f"{what}: axis {a} needs {2 * r + 1} taps, got {len(t)}")
            if any(t[r + k] != t[r - k] for k in range(1, r + 1)):
                raise ValueError(f"{what}: the taps must be symmetric")
            for k in range(r + 1):
                half[a * (GAUSS_MAX_RADIUS + 1) + k] = t[r + k]
    return radii, half


def _check_same_shape(I, J, what):
    """The image pair of a similarity (`what`: "lncc" or "mutual_information"), here and in similarity.py."""
    if J.shape != I.shape:
        raise RuntimeError(f"{what}: I {tuple(I.shape)} and J {tuple(J.shape)} must have the same shape")


def _check_lncc_pair(I, J):
    _check_tensors((("I", I), ("J", J)))
    _suffix(I)
    frame = _spatial_frame(I, "Only two- and three-dimensional lncc is supported")
    _check_same_shape(I, J, "lncc")
    _same(I, J)
    return frame


def _check_lncc_eps(eps):
    eps = float(eps)
    if not eps >= 0.0:
        raise ValueError(f"lncc: eps must not be negative (got {eps})")
    return eps


def lncc_moments(I, J, radii, taps, mode):
    """The five windowed moments (G I, G J, G(I I), G(I J), G(J J)) of I, J (N, C, *sp) as one (5, N, C, *sp) tensor
    (csrc/lncc.hip: lncc_moments_kernel along the last axis, then the pass kernels of gaussian_smooth over the stacked
    rows).  radii, taps, mode: as for gaussian_smooth_forward.  One scratch tensor like the result is allocated here
    when an axis besides the last is filtered.  Not in the reference; no CPU path."""
    dim, nx, ny, nz = _check_lncc_pair(I, J)
    radii, half = _gauss_half_taps("lncc", dim, radii, taps, mode)
    _check_cuda((("I", I),))
    I, J = I.contiguous(), J.contiguous()
    out = torch.empty((5,) + tuple(I.shape), dtype=I.dtype, device=I.device)
    scratch = torch.empty_like(out) if any(r > 0 for r in radii[:-1]) else None
    rad = (ctypes.c_int * dim)(*radii)
    _call("lago_lncc_moments", I, _ptr(out), _ptr(I), _ptr(J), _ptr(scratch), rad, half, GAUSS_MODES[mode], dim,
          I.size(0) * I.size(1), nx, ny, nz)
    return out


def lncc_cc(moments, eps):
    """cc = sX^2 / (sI sJ + eps) (N, C, *sp) from the moments of lncc_moments (csrc/lncc.hip: lncc_cc_kernel)."""
    _check_types((("moments", moments),))
    if moments.dim() not in (5, 6) or moments.size(0) != 5:
        raise RuntimeError(f"lncc_cc: moments must be (5, N, C, *spatial), got {tuple(moments.shape)}")
    eps = _check_lncc_eps(eps)
    _check_input(moments, "moments")
    cc = torch.empty(tuple(moments.shape[1:]), dtype=moments.dtype, device=moments.device)
    _call("lago_lncc_cc", moments, _ptr(cc), _ptr(moments), eps, cc.numel())
    return cc


def lncc_backward(grad_out, I, J, moments, radii, taps, mode, eps, need_I=True, need_J=True):
    """(dI, dJ) of cc = lncc for the upstream gradient grad_out, from the saved moments: the coefficient fields
    (lncc_coeff_kernel), ONE stacked gaussian_smooth_forward over them, and lncc_combine_kernel (csrc/lncc.hip).  A
    gradient that is not needed is None.  Not in the reference; no CPU path."""
    dim, nx, ny, nz = _check_lncc_pair(I, J)
    radii, _ = _gauss_half_taps("lncc", dim, radii, taps, mode)
    eps = _check_lncc_eps(eps)
    if not isinstance(grad_out, torch.Tensor) or not isinstance(moments, torch.Tensor):
        raise TypeError("grad_out and moments must be torch.Tensors")
    if grad_out.shape != I.shape or tuple(moments.shape) != (5,) + tuple(I.shape):
        raise RuntimeError("lncc_backward: grad_out must have the shape of I and moments be (5, *I.shape)")
    _same(I, grad_out, moments)
    if not (need_I or need_J):
        return None, None
    _check_cuda((("I", I),))
    I, J, grad_out, moments = I.contiguous(), J.contiguous(), grad_out.contiguous(), moments.contiguous()
    which = (1 if need_I else 0) | (2 if need_J else 0)
    k = 5 if which == 3 else 3
    n = I.numel()
    coef = torch.empty((k * I.size(0), I.size(1)) + tuple(I.shape[2:]), dtype=I.dtype, device=I.device)
    _call("lago_lncc_coeffs", I, _ptr(coef), _ptr(moments), _ptr(grad_out), eps, which, n)
    sm = gaussian_smooth_forward(coef, radii, taps, mode)
    del coef
    d_I = torch.empty_like(I) if need_I else None
    d_J = torch.empty_like(J) if need_J else None
    _call("lago_lncc_combine", I, _ptr(d_I), _ptr(d_J), _ptr(sm), _ptr(I), _ptr(J), which, n)
    return d_I, d_J


MI_MIN_BINS, MI_MAX_BINS, MI_FRAC_BITS = 4, 64, 32   # LAGO_MI_* of include/lagomorph_hip.h


def _check_mi(I, J, bins, range_I, range_J):
    """The checks mi_histogram and mi_backward share: (dim, nx, ny, nz, bins, (loI, hiI), (loJ, hiJ))."""
    _check_input(I, "I")
    _check_input(J, "J")
    _suffix(I)
    _same(I, J)
    frame = _spatial_frame(I, "Only two- and three-dimensional mutual information is supported")
    _check_same_shape(I, J, "mutual_information")
    return (*frame, mi_bins(bins), mi_range(range_I, "range_I"), mi_range(range_J, "range_J"))


def mi_bins(bins):
    if isinstance(bins, bool) or int(bins) != bins or not MI_MIN_BINS <= int(bins) <= MI_MAX_BINS:
        raise ValueError(f"mutual_information: bins must be an integer in {MI_MIN_BINS}..{MI_MAX_BINS} (got {bins!r})")
    return int(bins)


def mi_range(r, name):
    """(lo, hi) as floats; ValueError unless both are finite and lo < hi."""
    try:
        lo, hi = (float(v) for v in r)
    except (TypeError, ValueError):
        raise ValueError(f"mutual_information: {name} must be a pair (lo, hi) of numbers (got {r!r})") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError(f"mutual_information: {name} needs finite bounds lo < hi (got ({lo}, {hi}))")
    return lo, hi


def mi_histogram(I, J, bins, range_I, range_J):
    """The Parzen-window joint histogram P (N, C, bins, bins), float64, of I and J (N, C, *sp) over the ranges
    (lo, hi) of the two images: cubic B-spline windows on both, summed as 64-bit fixed-point integers, so that P has
    the same bits from call to call (csrc/mi.hip: mi_hist_kernel, csrc/chunk_table.hpp: table_reduce_kernel; the definition is in
    include/lagomorph_hip.h).  The scratch of partial tables is allocated here.  Not in the reference; no CPU path."""
    dim, nx, ny, nz, bins, (loI, hiI), (loJ, hiJ) = _check_mi(I, J, bins, range_I, range_J)
    rows, nvox = I.size(0) * I.size(1), nx * ny * nz
    P = torch.empty((I.size(0), I.size(1), bins, bins), dtype=torch.float64, device=I.device)
    tables = int(_lib.lago_mi_scratch_tables(bins, rows, nvox))
    scratch = torch.empty((rows * tables * bins * bins,), dtype=torch.int64, device=I.device)
    _call("lago_mi_histogram", I, _ptr(P), _ptr(I), _ptr(J), _ptr(scratch), tables, bins, loI, hiI, loJ, hiJ, dim, rows,
          nx, ny, nz)
    return P


def mi_backward(G, I, J, bins, range_I, range_J, need_I=True, need_J=True):
    """(dI, dJ) of mi_histogram for the upstream gradient G = dL/dP (N, C, bins, bins), float64: one gather pass from
    the row's table in LDS (csrc/mi.hip: mi_bwd_kernel).  A gradient that is not needed is None, neither computed nor
    written.  Not in the reference; no CPU path."""
    dim, nx, ny, nz, bins, (loI, hiI), (loJ, hiJ) = _check_mi(I, J, bins, range_I, range_J)
    _check_input(G, "G")
    if G.dtype != torch.float64 or G.device != I.device or tuple(G.shape) != (I.size(0), I.size(1), bins, bins):
        raise RuntimeError("mi_backward: G must be a float64 tensor (N, C, bins, bins) on the device of I")
    if not (need_I or need_J):
        return None, None
    d_I = torch.empty_like(I) if need_I else None
    d_J = torch.empty_like(J) if need_J else None
    _call("lago_mi_backward", I, _ptr(d_I), _ptr(d_J), _ptr(G), _ptr(I), _ptr(J), bins, loI, hiI, loJ, hiJ, dim,
          I.size(0) * I.size(1), nx, ny, nz)
    return d_I, d_J


LABEL_MODES = {"nearest": 0, "vote": 1}   # LAGO_LABELS_NEAREST / LAGO_LABELS_VOTE of include/lagomorph_hip.h
LABELS_MAX = 4096                         # LAGO_LABELS_MAX
_LABEL_DTYPES = (torch.uint8, torch.int16, torch.int32, torch.int64)


def label_mode(mode):
    if not isinstance(mode, str) or mode not in LABEL_MODES:
        raise ValueError(f"warp_labels: mode must be one of {sorted(LABEL_MODES)} (got {mode!r})")
    return LABEL_MODES[mode]


def label_count(num_labels):
    try:
        ok = not isinstance(num_labels, bool) and int(num_labels) == num_labels and 1 <= int(num_labels) <= LABELS_MAX
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"label_overlap: num_labels must be an integer in 1..{LABELS_MAX} (got {num_labels!r})")
    return int(num_labels)


def _check_labels(x, name):
    """A label map (N, 1, *sp) of an integer dtype; the device checks come last (_check_input), so that every error of
    shape, dtype, mode or label count is raised whatever device the tensors are on."""
    _check_tensors(((name, x),))
    if x.dtype not in _LABEL_DTYPES:
        raise RuntimeError(f"{name} must hold integer labels (uint8, int16, int32 or int64), got dtype {x.dtype}")
    if x.dim() not in (4, 5) or x.size(1) != 1:
        raise RuntimeError(f"{name} must be a label map of shape (N, 1, *spatial) with two or three spatial axes, "
                           f"got shape {tuple(x.shape)}")


def _as_int32(x):
    return x if x.dtype == torch.int32 else x.to(torch.int32)


def warp_labels(L, u, dt=1.0, mode="vote"):
    """out(x) = the label of L at x + dt u(x): L (N or 1, 1, *sp) integer label VALUES, u (N, d, *sp) float32 or
    float64, out (N, 1, *sp) in L's dtype.  mode "nearest" or "vote" (the label with the largest sum of multilinear
    corner weights, the smallest label among equal sums); the definition is in include/lagomorph_hip.h
    (csrc/labels.hip: warp_labels_kernel, warp_labels3_unroll_kernel).  The call takes int32: other dtypes are
    converted and converted back, and values of an int64 tensor outside the int32 range are the caller's error (not
    checked: that would synchronise).  Not differentiable.  Not in the reference; no CPU path."""
    mode = label_mode(mode)
    _check_labels(L, "L")
    _check_types((("u", u),))
    dim, nx, ny, nz = _spatial(L)
    if u.dim() != L.dim() or not _on_grid(u, L, dim):
        raise RuntimeError(f"warp_labels: displacement of shape {tuple(u.shape)} does not match labels {tuple(L.shape)}")
    nn = u.size(0)
    bc = _broadcast(L, nn, "warp_labels: batch sizes of L and u are incompatible", empty=True)
    if L.device != u.device:
        raise RuntimeError(f"lagomorph_ext: device mismatch ({L.device} vs {u.device})")
    _check_input(L, "L")
    _check_input(u, "u")
    L32 = _as_int32(L)
    out = torch.empty((nn, 1) + tuple(L.shape[2:]), dtype=torch.int32, device=L.device)
    _call("lago_warp_labels", u, _ptr(out), _ptr(L32), _ptr(u), float(dt), mode, int(bc), dim, nn, nx, ny, nz)
    return out if L.dtype == torch.int32 else out.to(L.dtype)


def label_overlap_chunks(num_labels, rows, nvox):
    """Partial tables per row label_overlap uses (lago_label_overlap_scratch_chunks)."""
    return int(_lib.lago_label_overlap_scratch_chunks(num_labels, rows, nvox))


def label_overlap(A, B, num_labels):
    """int64 counts (N, K, 3) of two label maps A, B (N, 1, *sp): per item and label k in [0, K = num_labels)
    [#(A == k), #(B == k), #(A == k and B == k)]; a voxel whose label is outside [0, K) counts in nothing for that
    image.  Integer sums in LDS tables and a slab of partial tables allocated here, no atomic on memory: the same
    bits from call to call (csrc/labels.hip: label_overlap_kernel, csrc/chunk_table.hpp: table_reduce_kernel).  Labels go to the
    call as int32 (see warp_labels).  Not in the reference; no CPU path."""
    K = label_count(num_labels)
    _check_labels(A, "A")
    _check_labels(B, "B")
    if B.shape != A.shape:
        raise RuntimeError(f"label_overlap: A {tuple(A.shape)} and B {tuple(B.shape)} must have the same shape")
    _same(A, B)
    _check_input(A, "A")
    _check_input(B, "B")
    rows, nvox = A.size(0), A[0].numel()
    A32 = _as_int32(A)
    B32 = A32 if B is A else _as_int32(B)
    counts = torch.empty((rows, K, 3), dtype=torch.int64, device=A.device)
    chunks = label_overlap_chunks(K, rows, nvox)
    scratch = torch.empty((rows * chunks * K * 3,), dtype=torch.int32, device=A.device)
    _launch(_lib.lago_label_overlap, A, _ptr(counts), _ptr(A32), _ptr(B32), _ptr(scratch), chunks, K, rows, nvox)
    return counts


EDT_WHERE = {"nonzero": 0, "equal": 1, "not_equal": 2, "surface": 3}   # LAGO_EDT_* of include/lagomorph_hip.h
EDT_MAX_EXTENT = 1024                                                  # LAGO_EDT_MAX_EXTENT


def edt_where(where):
    if not isinstance(where, str) or where not in EDT_WHERE:
        raise ValueError(f"distance_transform: where must be one of {sorted(EDT_WHERE)} (got {where!r})")
    return EDT_WHERE[where]


def edt_spacing(spacing, dim):
    """One positive float, or one per spatial axis, as a tuple of `dim` floats that are positive and finite in float32
    (what the kernels compute in)."""
    try:
        sp = (float(spacing),) * dim if not hasattr(spacing, "__len__") else tuple(float(s) for s in spacing)
    except (TypeError, ValueError):
        raise ValueError(f"distance_transform: spacing must be a positive float or one per axis (got {spacing!r})") from None
    if len(sp) != dim:
        raise ValueError(f"distance_transform: spacing must have one entry per spatial axis ({dim}), got {len(sp)}")
    for s in sp:
        if not (s > 0.0 and math.isfinite(s) and 1e-38 < s < 3e38):
            raise ValueError(f"distance_transform: spacing must be positive and finite in float32 (got {spacing!r})")
    return sp


def distance_transform(L, where="nonzero", label=0, spacing=1.0, squared=False):
    """float32 (N, 1, *sp): the Euclidean distance (squared=True: its square) from every voxel to the nearest feature
    voxel of its item; L (N, 1, *sp) integer or bool labels, features by `where` ("nonzero", "equal", "not_equal",
    "surface" of `label`); the definition is in include/lagomorph_hip.h (csrc/edt.hip: edt_pass_kernel, one launch per
    axis, no scratch buffer).  The call takes int32 (see warp_labels).  Not in the reference; no CPU path."""
    where = edt_where(where)
    _check_tensors((("L", L),))
    if L.dtype != torch.bool:
        _check_labels(L, "L")
    elif L.dim() not in (4, 5) or L.size(1) != 1:
        raise RuntimeError(f"L must be a label map of shape (N, 1, *spatial) with two or three spatial axes, got shape {tuple(L.shape)}")
    try:
        ok = not isinstance(label, bool) and int(label) == label and -2**31 <= int(label) < 2**31
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"distance_transform: label must be an integer in the int32 range (got {label!r})")
    dim, nx, ny, nz = _spatial(L)
    sp = edt_spacing(spacing, dim)
    if max(L.shape[2:]) > EDT_MAX_EXTENT:
        raise RuntimeError(f"distance_transform: extents up to {EDT_MAX_EXTENT} are supported, got shape {tuple(L.shape)}")
    _check_input(L, "L")
    L32 = _as_int32(L)
    out = torch.empty(L.shape, dtype=torch.float32, device=L.device)
    _launch(_lib.lago_distance_transform, L, _ptr(out), _ptr(L32), where, int(label), (_dbl * dim)(*sp), int(bool(squared)), dim,
            L.size(0), nx, ny, nz)
    return out


def _check_points(F, x, what, grad_out=None, backward=False):
    """A field F (N or 1, C, *sp) with two or three spatial axes and a point set x (N, d, P), d = len(sp), of one
    floating dtype (and, for the backward, grad_out (N, C, P)); returns (dim, nx, ny, nz, nn, broadcast).  Every error of type,
    dtype, shape, batch and contiguity is raised whatever device the tensors are on; the device checks come last."""
    named = (("F", F), ("x", x)) + ((("grad_out", grad_out),) if backward else ())
    _check_types(named)
    dim, nx, ny, nz = _spatial_frame(F, f"{what}: F must be a field of shape (N, C, *spatial) with two or three spatial "
                                        f"axes, got shape {tuple(F.shape)}")
    if x.dim() != 3 or x.size(1) != dim:
        raise RuntimeError(f"{what}: x must be a point set of shape (N, {dim}, P) for a field with {dim} spatial axes, "
                           f"got shape {tuple(x.shape)}")
    nn = x.size(0)
    bc = _broadcast(F, nn, f"{what}: batch sizes of F ({F.size(0)}) and x ({nn}) are incompatible", empty=True)
    if backward and tuple(grad_out.shape) != (nn, F.size(1), x.size(2)):
        raise RuntimeError(f"{what}: grad_out of shape {tuple(grad_out.shape)} does not match the output "
                           f"{(nn, F.size(1), x.size(2))}")
    _check_layout(named)
    return dim, nx, ny, nz, nn, bc


def interp_points_forward(F, x):
    """out (N, C, P): F (N or 1, C, *sp) sampled multilinearly at the positions x (N, d, P), in voxel-index units;
    lago_interp_points of include/lagomorph_hip.h (csrc/points.hip: interp_points_fwd_kernel).  Not in the reference;
    no CPU path."""
    dim, nx, ny, nz, nn, bc = _check_points(F, x, "interp_points")
    out = torch.empty((nn, F.size(1), x.size(2)), dtype=F.dtype, device=F.device)
    _call("lago_interp_points", F, _ptr(out), _ptr(F), _ptr(x), dim, nn, F.size(1), x.size(2), nx, ny, nz, int(bc))
    return out


def interp_points_backward(grad_out, F, x, need_F, need_x):
    """[d_F like F or None, d_x like x or None] for grad_out (N, C, P): lago_interp_points_backward
    (csrc/points.hip: interp_points_bwd_kernel).  A gradient that is not needed is not computed.  d_F is a sum of
    hardware float atomics (its last bits differ from call to call), d_x repeats bit for bit."""
    dim, nx, ny, nz, nn, bc = _check_points(F, x, "interp_points_backward", grad_out, backward=True)
    d_F = torch.empty_like(F) if need_F else None
    d_x = torch.empty_like(x) if need_x else None
    if need_F or need_x:
        _call("lago_interp_points_backward", F, _ptr(d_F), _ptr(d_x), _ptr(grad_out), _ptr(F), _ptr(x), dim, nn,
              F.size(1), x.size(2), nx, ny, nz, int(bc), int(bool(need_F)), int(bool(need_x)))
    return [d_F, d_x]


def bspline_prefilter(I, adjoint=False):
    """Cubic B-spline coefficients (N, C, *sp) of the samples I (N, C, *sp), mirror border; adjoint: the transposed
    operator.  lago_bspline_prefilter of include/lagomorph_hip.h (csrc/bspline.hip).  Not in the reference; no CPU path."""
    _check_types((("I", I),))
    dim, nx, ny, nz = _spatial_frame(I, "bspline_prefilter: I must be a field of shape (N, C, *spatial) with two or three "
                                        f"spatial axes, got shape {tuple(I.shape)}")
    _check_layout((("I", I),))
    out = torch.empty_like(I)
    _call("lago_bspline_prefilter", I, _ptr(out), _ptr(I), int(bool(adjoint)), dim, I.size(0) * I.size(1), nx, ny, nz)
    return out


def _check_bspline(C, u, what, grad_out=None):
    """Coefficients C (N or 1, K, *sp) with two or three spatial axes and a displacement u (N, d, *sp) of one floating
    dtype (and, for the backward, grad_out (N, K, *sp)); returns (dim, nx, ny, nz, nn, broadcast).  Every error of type,
    dtype, shape, batch and contiguity is raised whatever device the tensors are on; the device checks come last."""
    named = (("C", C), ("u", u)) + ((("grad_out", grad_out),) if grad_out is not None else ())
    _check_types(named)
    dim, nx, ny, nz = _spatial_frame(C, f"{what}: C must be a field of shape (N, K, *spatial) with two or three spatial "
                                        f"axes, got shape {tuple(C.shape)}")
    if u.dim() != C.dim() or not _on_grid(u, C, dim):
        raise RuntimeError(f"{what}: displacement of shape {tuple(u.shape)} does not match the field {tuple(C.shape)}")
    nn = u.size(0)
    bc = _broadcast(C, nn, f"{what}: batch sizes of C ({C.size(0)}) and u ({nn}) are incompatible", empty=True)
    if grad_out is not None and tuple(grad_out.shape) != (nn, C.size(1)) + tuple(C.shape[2:]):
        raise RuntimeError(f"{what}: grad_out of shape {tuple(grad_out.shape)} does not match the output "
                           f"{(nn, C.size(1)) + tuple(C.shape[2:])}")
    _check_layout(named)
    return dim, nx, ny, nz, nn, bc


def interp_bspline_forward(C, u, dt=1.0):
    """out (N, K, *sp): the cubic B-spline with coefficients C (N or 1, K, *sp) at i + dt u(i); lago_interp_bspline
    (csrc/bspline.hip: interp_bspline_fwd_kernel).  Not in the reference; no CPU path."""
    dim, nx, ny, nz, nn, bc = _check_bspline(C, u, "interp_bspline")
    out = torch.empty((nn, C.size(1)) + tuple(C.shape[2:]), dtype=C.dtype, device=C.device)
    _call("lago_interp_bspline", C, _ptr(out), _ptr(C), _ptr(u), float(dt), dim, nn, C.size(1), nx, ny, nz, int(bc))
    return out


def interp_bspline_backward(grad_out, C, u, dt, need_C, need_u):
    """[d_C like C or None, d_u like u or None] for grad_out (N, K, *sp): lago_interp_bspline_backward
    (csrc/bspline.hip: interp_bspline_bwd_kernel).  A gradient that is not needed is not computed.  d_C is a sum of
    hardware float atomics (its last bits differ from call to call), d_u repeats bit for bit."""
    dim, nx, ny, nz, nn, bc = _check_bspline(C, u, "interp_bspline_backward", grad_out)
    d_C = torch.empty_like(C) if need_C else None
    d_u = torch.empty_like(u) if need_u else None
    if need_C or need_u:
        _call("lago_interp_bspline_backward", C, _ptr(d_C), _ptr(d_u), _ptr(grad_out), _ptr(C), _ptr(u), float(dt), dim, nn,
              C.size(1), nx, ny, nz, int(bc), int(bool(need_C)), int(bool(need_u)))
    return [d_C, d_u]


FFD_MAX_SPACING = 32   # spacings lago_ffd_expand takes: 1..32 voxels


def ffd_spacing(spacing, dim):
    """`spacing` as a tuple of `dim` integers: one integer for every axis, or one per axis.  RuntimeError otherwise."""
    sp = (spacing,) * dim if isinstance(spacing, int) and not isinstance(spacing, bool) else spacing
    try:
        sp = tuple(sp)
        ok = len(sp) == dim and all(isinstance(v, int) and not isinstance(v, bool) and 1 <= v <= FFD_MAX_SPACING for v in sp)
    except TypeError:
        ok = False
    if not ok:
        raise RuntimeError(f"ffd: spacing must be one integer in 1..{FFD_MAX_SPACING}, or one per spatial axis ({dim}), "
                           f"got {spacing!r}")
    return sp


def ffd_grid_shape(shape, spacing):
    """Control-lattice extents for a field of spatial `shape` (two or three extents >= 1): (n - 1) // s + 4 per axis."""
    try:
        shape = tuple(shape)
        ok = len(shape) in (2, 3) and all(isinstance(n, int) and not isinstance(n, bool) and n >= 1 for n in shape)
    except TypeError:
        ok = False
    if not ok:
        raise RuntimeError(f"ffd: shape must give two or three spatial axes with extents >= 1, got {shape!r}")
    return tuple((n - 1) // s + 4 for n, s in zip(shape, ffd_spacing(spacing, len(shape))))


def _check_ffd(x, shape, spacing, what):
    """A control lattice x (N, C, *m) with the field's spatial `shape` (forward), or a field x (N, C, *sp) with shape
    None (adjoint); returns (dim, field shape, spacing tuple).  Every error of type, dtype, shape and contiguity is
    raised whatever device the tensor is on; the device checks come last."""
    name = "ctrl" if shape is not None else "g"
    _check_types(((name, x),))
    dim = _spatial_frame(x, f"{what}: {name} must be a field of shape (N, C, *spatial) with two or three spatial axes, "
                            f"got shape {tuple(x.shape)}")[0]
    if shape is None:
        shape = tuple(x.shape[2:])
        if min(shape) < 1:
            raise RuntimeError(f"{what}: g of shape {tuple(x.shape)} has an empty spatial axis")
    else:
        try:
            shape = tuple(shape)
        except TypeError:
            raise RuntimeError(f"ffd: shape must give two or three spatial axes with extents >= 1, got {shape!r}") from None
        if len(shape) != dim:
            raise RuntimeError(f"{what}: a control grid of shape {tuple(x.shape)} does not match a field with "
                               f"{len(shape)} spatial axes ({shape})")
    sp = ffd_spacing(spacing, dim)
    if name == "ctrl" and tuple(x.shape[2:]) != ffd_grid_shape(shape, sp):
        raise RuntimeError(f"{what}: a control grid of shape {tuple(x.shape)} does not match the field {shape} at spacing "
                           f"{sp}: its spatial extents must be {ffd_grid_shape(shape, sp)}")
    _check_layout(((name, x),))
    return dim, shape, sp


def ffd_expand(ctrl, shape, spacing):
    """out (N, C, *shape): the control lattice ctrl (N, C, *ffd_grid_shape(shape, spacing)) expanded by its uniform
    cubic B-spline; lago_ffd_expand of include/lagomorph_hip.h (csrc/ffd.hip: ffd_expand_kernel).  No atomics: the
    same bits from call to call.  Not in the reference; no CPU path."""
    dim, shape, sp = _check_ffd(ctrl, shape, spacing, "ffd_expand")
    out = torch.empty(tuple(ctrl.shape[:2]) + shape, dtype=ctrl.dtype, device=ctrl.device)
    _call("lago_ffd_expand", ctrl, _ptr(out), _ptr(ctrl), dim, ctrl.size(0) * ctrl.size(1), *_pad(shape, 1), *_pad(sp, 1))
    return out


def ffd_expand_adjoint(g, spacing):
    """d_ctrl (N, C, *ffd_grid_shape(g.shape[2:], spacing)) for g (N, C, *sp): the transpose of ffd_expand;
    lago_ffd_expand_adjoint (csrc/ffd.hip: ffd_restrict_tile_kernel, ffd_restrict_sum_kernel).  The scratch of
    per-tile partial sums is allocated here.  No atomic on memory: the same bits from call to call, and control points
    that no voxel reaches hold exactly 0."""
    dim, shape, sp = _check_ffd(g, None, spacing, "ffd_expand_adjoint")
    rows = g.size(0) * g.size(1)
    d_ctrl = torch.empty(tuple(g.shape[:2]) + ffd_grid_shape(shape, sp), dtype=g.dtype, device=g.device)
    n, s = _pad(shape, 1), _pad(sp, 1)
    elems = _scratch_elems(_lib.lago_ffd_scratch_elems, dim, rows, *n, *s)
    scratch = torch.empty((elems,), dtype=g.dtype, device=g.device)
    _call("lago_ffd_expand_adjoint", g, _ptr(d_ctrl), _ptr(g), _ptr(scratch), elems, dim, rows, *n, *s)
    return d_ctrl


def _check_luts(what, ref, cosluts, sinluts, lengths):
    """The cosine and sine LUT of every axis, of ref's dtype and device and of that axis's length in `lengths`, made
    contiguous: [cos 0, sin 0, cos 1, ...] (the caller keeps the list alive over its launch)."""
    luts = []
    for d, n in enumerate(lengths):
        for t in (cosluts[d], sinluts[d]):
            if t.dtype != ref.dtype:
                raise RuntimeError("Type of LUTs must equal that of image")
            if not t.is_cuda or t.device != ref.device or t.numel() != n:
                raise RuntimeError(f"{what}: LUT on wrong device or of wrong length")
            luts.append(t.contiguous())
    return luts


def fluid_operator(Fmv, inverse, cosluts, sinluts, alpha, beta, gamma):
    """extension.cpp:158-173 -> cuda/metric.cu:308-355.  In place on Fmv (N, d, nx, ny[, nzc], 2)."""
    _check_input(Fmv, "Fmv")
    dim = Fmv.dim() - 3
    if len(cosluts) != dim:
        raise RuntimeError(f"Must provide same number cosine LUTs ({len(cosluts)}) as spatial dimension '{dim}'")
    if len(sinluts) != dim:
        raise RuntimeError(f"Must provide same number sine LUTs ({len(sinluts)}) as spatial dimension '{dim}'")
    if dim not in (2, 3):
        raise RuntimeError("Only two- and three-dimensional fluid metric is supported")
    if Fmv.size(1) != dim or Fmv.size(-1) != 2:
        raise RuntimeError("Vector field has incorrect shape for dimension")
    sh = Fmv.shape[2:2 + dim]
    luts = _check_luts("fluid_operator", Fmv, cosluts, sinluts, sh)
    _call("lago_fluid_operator", Fmv, _ptr(Fmv), int(bool(inverse)), *_pad([_ptr(t) for t in luts], None, 6), float(alpha),
          float(beta), float(gamma), dim, Fmv.size(0), *_pad(sh, 1))
    return None


def fluid_cache_clear():
    """Drop the library's cached per-frequency coefficient tables."""
    _lib.lago_fluid_cache_clear()


def fluid_cache_entries():
    return int(_lib.lago_fluid_cache_entries())


def fft_plan_state():
    """(cached rocFFT fallback plans, how many of them are currently verified by the spot check)."""
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    _lib.lago_fft_plan_state(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def fluid_metric(mv, inverse, cosluts, sinluts, alpha, beta, gamma, lut_generation=0, out_scale=1.0):
    """Whole FluidMetricOperator.forward (metric.py:11-19) in one call: irfft(L^(+-2) rfft(mv)).
    Not part of the reference's extension surface.  Returns a new tensor; mv is not modified.
    `lut_generation` names the CONTENTS of the LUTs (see include/lagomorph_hip.h): non-zero lets the
    library cache its coefficient table under that number; 0 takes the table-free path.
    `out_scale`: a factor on the result, applied to the finished value (the bits of `result * out_scale`) inside the
    last kernel where that kernel can take it (lago_fluid_metric_scaled)."""
    _check_input(mv, "mv")
    dim, nx, ny, nz = _spatial_frame(mv, "Only two- and three-dimensional fluid metric is supported")
    if mv.size(1) != dim:
        raise RuntimeError("Vector field has incorrect shape for dimension")
    if len(cosluts) != dim or len(sinluts) != dim:
        raise RuntimeError(f"Must provide same number of LUTs as spatial dimension '{dim}'")
    csh = list(mv.shape[2:])
    csh[-1] = csh[-1] // 2 + 1
    luts = _check_luts("fluid_metric", mv, cosluts, sinluts, csh)
    out = torch.empty_like(mv)
    work = torch.empty((mv.size(0), dim, *csh, 2), dtype=mv.dtype, device=mv.device)
    p = _pad([_ptr(t) for t in luts], None, 6)
    if float(out_scale) != 1.0:
        _call("lago_fluid_metric_scaled", mv, _ptr(out), _ptr(mv), _ptr(work), int(lut_generation), int(bool(inverse)), *p,
              float(alpha), float(beta), float(gamma), dim, mv.size(0), nx, ny, nz, float(out_scale))
        return out
    _call("lago_fluid_metric", mv, _ptr(out), _ptr(mv), _ptr(work), int(lut_generation), int(bool(inverse)), *p, float(alpha), float(beta),
          float(gamma), dim, mv.size(0), nx, ny, nz)
    return out


_AFFINE_DIMS = "Only two- and three-dimensional affine interpolation is supported"


def affine_interp_forward(I, A, T):
    """extension.cpp:109-118 -> cuda/affine.cu:114-169.  The reference falls back to
    cpu/affine.cpp for CPU tensors; this build is HIP-only and raises instead."""
    _check_input(I, "I")
    _check_input(A, "A")
    _check_input(T, "T")
    _same(I, A, T)
    if A.size(0) != T.size(0):
        raise RuntimeError("A and T must have same first dimension")
    dim, nx, ny, nz = _spatial_frame(I, _AFFINE_DIMS)
    if tuple(A.shape[1:]) != (dim, dim) or tuple(T.shape[1:]) != (dim,):
        raise RuntimeError("affine_interp_forward: A must be (N, d, d) and T (N, d)")
    nn = A.size(0)
    bc = _broadcast(I, nn, "affine_interp_forward: batch sizes of I and A are incompatible")
    out = torch.empty((nn, I.size(1)) + tuple(I.shape[2:]), dtype=I.dtype, device=I.device)
    _call("lago_affine_interp_forward", I, _ptr(out), _ptr(I), _ptr(A), _ptr(T), dim, nn, I.size(1), nx, ny, nz, int(bc))
    return out


def affine_interp_backward(grad_out, I, A, T, need_I, need_A, need_T):
    """extension.cpp:120-133 -> cuda/affine.cu:538-610.  Unneeded gradients are size-0 tensors."""
    _check_input(grad_out, "grad_out")
    _check_input(I, "I")
    _check_input(A, "A")
    _check_input(T, "T")
    _same(I, A, T, grad_out)
    if I.size(1) != grad_out.size(1):
        raise RuntimeError("I and grad_out must have same number of channels")
    if A.size(0) != T.size(0):
        raise RuntimeError("A and T must have same first dimension")
    dim, nx, ny, nz = _spatial_frame(I, _AFFINE_DIMS)
    nn = grad_out.size(0)
    inconsistent = "affine_interp_backward: grad_out / I / A shapes are inconsistent"
    if A.size(0) != nn or tuple(grad_out.shape[2:]) != tuple(I.shape[2:]):
        raise RuntimeError(inconsistent)
    bc = _broadcast(I, nn, inconsistent)
    empty = lambda: torch.zeros((0,), dtype=I.dtype, device=I.device)
    d_I = torch.empty_like(I) if need_I else empty()
    d_A = torch.empty_like(A) if need_A else empty()
    d_T = torch.empty_like(T) if need_T else empty()
    _call("lago_affine_interp_backward", I, _ptr(d_I), _ptr(d_A), _ptr(d_T), _ptr(grad_out), _ptr(I), _ptr(A), _ptr(T),
          dim, nn, I.size(1), nx, ny, nz, int(bc), int(bool(need_I)), int(bool(need_A)), int(bool(need_T)))
    return [d_I, d_A, d_T]


def compose(u, v, ds=1.0, dt=1.0, out=None, near_identity=False):
    """Fused deform.compose (deform.py:53-55): ds*u + dt*interp(v, u, dt=ds) in one kernel.
    Not part of the reference's extension surface; u and v are (N, d, *spatial) vector fields.  `out`: a contiguous
    tensor of their shape to write into (it must not alias u or v).  `near_identity`: a hint that |ds*u| stays below one
    voxel (the Euler step of a shoot); it selects a kernel (`set_compose_near`), never a value."""
    _check_inputs((("u", u), ("v", v)))
    dim, nx, ny, nz = _spatial_frame(u, "Only two- and three-dimensional interpolation is supported")
    if u.shape != v.shape or u.size(1) != dim:
        raise RuntimeError("compose: u and v must be vector fields of the same shape")
    if out is None:
        out = torch.empty_like(u)
    else:
        _check_dest(out, "out", u, "compose: out must have the shape of u and must not alias an input", u, v)
    _call("lago_compose_near" if near_identity else "lago_compose", u, _ptr(out), _ptr(u), _ptr(v), float(ds), float(dt), dim,
          u.size(0), nx, ny, nz)
    return out


def lincomb(terms, out=None):
    """out = c0*x0 + c1*x1 + ... for 1 to 4 (coefficient, tensor) pairs of one shape and dtype, in one pass
    (left to right, one fma per term).  `out` may be one of the inputs (in place); a new tensor otherwise.
    Not part of the reference's extension surface: the elementwise sums of lddmm_step (lddmm.py:300-325)."""
    if not 1 <= len(terms) <= 4:
        raise RuntimeError("lincomb: 1 to 4 terms")
    xs = [x for _, x in terms]
    for x in xs:
        _check_input(x, "x")
        _same(xs[0], x)
        if x.shape != xs[0].shape:
            raise RuntimeError("lincomb: shapes differ")
    if out is None:
        out = torch.empty_like(xs[0])
    else:
        _check_dest(out, "out", xs[0], "lincomb: shapes differ")
    _call("lago_lincomb", xs[0], _ptr(out), len(terms), *_pad([_ptr(x) for x in xs], None, 4),
          *_pad([float(c) for c, _ in terms], 0.0, 4), xs[0].numel())
    return out


def interp_backward_fused(grad_out, I, u, dt, need_I, d_u=None, addgo=None, d_I=None):
    """interp_backward whose d_u sum starts from the contents of `d_u` (given: accumulated in place and returned)
    or from addgo * grad_out (needs as many channels as dimensions) instead of zero -- the chain-rule additions of
    compose's and Ad_star's backward without their extra passes; with `d_I` given the splat is added onto it
    instead of onto zeros.  Returns [d_I, d_u].  Not part of the reference's extension surface
    (include/lagomorph_hip.h: lago_interp_backward_fused)."""
    dim, nx, ny, nz, nn, bc = _interp_backward_args(grad_out, I, u)
    if (d_u is None) == (addgo is None):
        raise RuntimeError("interp_backward_fused: give exactly one of d_u (accumulate) and addgo")
    if d_u is not None:
        _check_dest(d_u, "d_u", u, "interp_backward_fused: d_u must have the shape of u")
        mode, ag = 1, 0.0
    else:
        if I.size(1) != dim:
            raise RuntimeError("interp_backward_fused: addgo needs as many channels as dimensions")
        d_u = torch.empty_like(u)
        mode, ag = 2, float(addgo)
    imode = 0
    if d_I is not None:
        _check_dest(d_I, "d_I", I, "interp_backward_fused: d_I must have the shape of I (and need_I be set)")
        if not need_I:
            raise RuntimeError("interp_backward_fused: d_I must have the shape of I (and need_I be set)")
        imode = 1
    else:
        d_I = torch.empty_like(I)
    _call("lago_interp_backward_fused", I, _ptr(d_I), _ptr(d_u), _ptr(grad_out), _ptr(I), _ptr(u), float(dt), dim, nn,
          I.size(1), nx, ny, nz, int(bc), int(bool(need_I)), imode, mode, ag)
    return [d_I, d_u]


def Ad_star(phiinv, m, save_resampled=False):
    """Fused adjrep.Ad_star (adjrep.py:86-97): jacobian_times_vectorfield(phiinv, interp(m, phiinv),
    displacement=True) in one kernel.  Not part of the reference's extension surface.  With save_resampled the
    resampled momentum interp(m, phiinv) is returned as well: (out, mphiinv)."""
    _check_inputs((("phiinv", phiinv), ("m", m)))
    dim, nx, ny, nz = _spatial_frame(phiinv, "Only two- and three-dimensional fields are supported")
    if phiinv.shape != m.shape or m.size(1) != dim:
        raise RuntimeError("Ad_star: phiinv and m must be vector fields of the same shape")
    out = torch.empty_like(m)
    mphi = torch.empty_like(m) if save_resampled else None
    _call("lago_Ad_star", m, _ptr(out), _ptr(mphi), _ptr(phiinv), _ptr(m), dim, m.size(0), nx, ny, nz)
    return (out, mphi) if save_resampled else out


def ad_star(v, m):
    """Fused adjrep.ad_star (adjrep.py:69-83): jacobian_times_vectorfield(v, m, transpose=True) minus
    jacobian_times_vectorfield_adjoint(m, v) in one kernel.  Not part of the reference's extension surface."""
    _check_inputs((("v", v), ("m", m)))
    dim, nx, ny, nz = _spatial_frame(v, _JTV_DIMS)
    if v.shape != m.shape or m.size(1) != dim:
        raise RuntimeError("ad_star: v and m must be vector fields of the same shape")
    out = torch.empty_like(m)
    _call("lago_ad_star", m, _ptr(out), _ptr(v), _ptr(m), dim, m.size(0), nx, ny, nz)
    return out


_REGRID_DIMS = "Only two- and three-dimensional regridding is supported"


def _vec3(x, dim, what):
    x = list(x)
    if len(x) != dim:
        raise RuntimeError(f"{what} should be vector of size d (not 2+d)")
    return (ctypes.c_double * 3)(*_pad([float(v) for v in x], 0.0))


def regrid_forward(I, shape, origin, spacing):
    """cuda/affine.cu:683-734"""
    _check_input(I, "I")
    dim, nx, ny, nz = _spatial_frame(I, _REGRID_DIMS)
    shape = [int(s) for s in shape]
    if len(shape) != dim:
        raise RuntimeError("Shape should be vector of size d (not 2+d)")
    O, S = _vec3(origin, dim, "Origin"), _vec3(spacing, dim, "Spacing")
    out = torch.empty(tuple(I.shape[:2]) + tuple(shape), dtype=I.dtype, device=I.device)
    _call("lago_regrid_forward", I, _ptr(out), _ptr(I), dim, I.size(0), I.size(1), nx, ny, nz, *_pad(shape, 1), O, S)
    return out


# 1 (default): regrid_backward runs axis by axis in gather form (lago_regrid_backward_sep: no atomics, no memset, results
# independent of the launch); 0: the reference's splat (LDS-privatised / global atomics by lago_tuning.splat_mode)
REGRID_BACKWARD_SEPARABLE = 1


def regrid_backward(grad_out, inshape, shape, origin, spacing):
    """cuda/affine.cu:802-855"""
    _check_input(grad_out, "grad_out")
    dim = _spatial_frame(grad_out, _REGRID_DIMS)[0]
    inshape = [int(s) for s in inshape]
    shape = [int(s) for s in shape]
    if len(inshape) != dim:
        raise RuntimeError("Input shape should be vector of size d (not 2+d)")
    if len(shape) != dim or list(grad_out.shape[2:]) != shape:
        raise RuntimeError("Shape should be vector of size d (not 2+d)")
    O, S = _vec3(origin, dim, "Origin"), _vec3(spacing, dim, "Spacing")
    n3, N = _pad(inshape, 1), _pad(shape, 1)
    d_I = torch.empty(tuple(grad_out.shape[:2]) + tuple(inshape), dtype=grad_out.dtype, device=grad_out.device)
    if REGRID_BACKWARD_SEPARABLE and all(S[d] > 0 for d in range(dim)) and d_I.numel() and grad_out.numel():
        # axis by axis in gather form (no atomics, deterministic): two temporaries, each as large as the biggest
        # intermediate (the axes go from grad_out's extents to d_I's one at a time, slowest axis first)
        planes = grad_out.size(0) * grad_out.size(1)
        cur, half = list(shape), 0
        for a in range(dim - 1):
            cur[a] = inshape[a]
            half = max(half, planes * math.prod(cur))
        ws = torch.empty((2 * half,), dtype=grad_out.dtype, device=grad_out.device) if half else None
        _call("lago_regrid_backward_sep", grad_out, _ptr(d_I), _ptr(grad_out), _ptr(ws), 2 * half, dim, grad_out.size(0),
              grad_out.size(1), n3[0], n3[1], n3[2], N[0], N[1], N[2], O, S)
        return d_I
    _call("lago_regrid_backward", grad_out, _ptr(d_I), _ptr(grad_out), dim, grad_out.size(0), grad_out.size(1), n3[0],
          n3[1], n3[2], N[0], N[1], N[2], O, S)
    return d_I
