"""Smoothness penalties on a field itself: the diffusion energy (VoxelMorph's) and the bending energy (Rueckert et al.
1999; NiftyReg, elastix), each one fused kernel pass with a fused backward, for registration loops that optimise a dense
displacement or an FFD lattice against a similarity.

    u = ffd_expand(c, I.shape[2:], spacing)
    loss = lncc_loss(interp(I, u), J) + lam * bending_energy(u).mean()     # the gradient reaches c through ffd_restrict

Fields are channel-first (N, C, *sp) with two or three spatial axes, float32 or float64, contiguous, on the GPU; C is free
(d channels for a displacement, 1 for a bias field).  `spacing` is the voxel size h_a per axis, a positive finite number
or one per axis, default 1.0.  Per item n, summed over the channels k, with V = prod(sp) the voxels of one item:

    diffusion   E = (1/V) sum_x sum_k sum_a (d_a u_k(x))^2
                d_a u(x) = (u(x + e_a) - u(x)) / h_a where x_a + 1 < n_a, 0 otherwise: a forward difference with a
                Neumann border; an axis of extent 1 contributes nothing
    bending     E = (1/V) sum_x sum_k [ sum_a (d_aa u_k(x))^2 + 2 sum_{a<b} (d_ab u_k(x))^2 ]
                d_aa u(x) = (u(x + e_a) - 2 u(x) + u(x - e_a)) / h_a^2 where 1 <= x_a <= n_a - 2, 0 otherwise
                d_ab u(x) = (u(x + e_a + e_b) - u(x + e_a) - u(x + e_b) + u(x)) / (h_a h_b) where x_a + 1 < n_a and
                x_b + 1 < n_b, 0 otherwise; axes of extent 1 or 2 drop their terms

Both are quadratic forms E = <u, A u> / V with A = sum_t w_t D_t^T D_t symmetric positive semidefinite, and
dE/du = (2/V) A u exactly, at the borders too.  Away from the borders A is -Laplacian (7-point) for diffusion and the
discrete biharmonic operator (25-point in 3D, 13-point in 2D) for bending.  The kernels use no atomics: the bits repeat
from call to call, on any stream.  No counterpart in the reference; no CPU path.
"""
import ctypes
import math

import torch

from . import lagomorph_ext as _ext

__all__ = ["EnergyOperatorFunction", "FieldEnergyFunction", "bending_energy", "diffusion_energy", "energy_operator",
           "field_energy"]

_KINDS = {"diffusion": 0, "bending": 1}   # LAGO_ENERGY_DIFFUSION, LAGO_ENERGY_BENDING


def _kind(kind):
    if not isinstance(kind, str) or kind not in _KINDS:
        raise RuntimeError(f"field_energy: kind must be one of {sorted(_KINDS)} (got {kind!r})")
    return _KINDS[kind]


def _spacing(spacing, dim):
    """`spacing` as a tuple of `dim` positive finite floats: one number for every axis, or one per axis."""
    sp = ()
    try:
        given = tuple(spacing) if hasattr(spacing, "__len__") and not isinstance(spacing, str) else (spacing,) * dim
        ok = len(given) == dim and not any(isinstance(s, (bool, str)) for s in given)
        if ok:
            sp = tuple(float(s) for s in given)
            ok = all(s > 0.0 and math.isfinite(s) for s in sp)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise RuntimeError(f"field_energy: spacing must be a positive finite number, or one per spatial axis ({dim}), got {spacing!r}")
    return sp


def _check(u, kind, spacing, what, scale=None):
    """A field u (N, C, *sp) and the optional scale (N,); returns (kind id, dim, spacing tuple).  Every error of type,
    dtype, shape and contiguity is raised whatever device the tensors are on; the device checks come last."""
    _ext._check_types((("u", u),))
    if scale is not None and not isinstance(scale, torch.Tensor):
        raise TypeError("scale must be a torch.Tensor or None")
    k = _kind(kind)
    dim = _ext._spatial_frame(u, f"{what}: u must be a field of shape (N, C, *spatial) with two or three spatial axes, "
                                 f"got shape {tuple(u.shape)}")[0]
    sp = _spacing(spacing, dim)
    named = (("u", u),)
    if scale is not None:
        if scale.dtype != u.dtype or tuple(scale.shape) != (u.size(0),):
            raise RuntimeError(f"{what}: scale must have u's dtype and the shape (N,) = ({u.size(0)},), got {scale.dtype} {tuple(scale.shape)}")
        named += (("scale", scale),)
    _ext._check_layout(named)
    return k, dim, sp


def _energy(u, kind, spacing):
    """E (N,) by lago_field_energy (csrc/energy.hip: energy_tile_kernel, energy_sum_kernel); the scratch of per-tile
    partial sums is allocated here."""
    k, dim, sp = _check(u, kind, spacing, "field_energy")
    N, C = u.size(0), u.size(1)
    if u.numel() == 0:
        return torch.zeros((N,), dtype=u.dtype, device=u.device)
    n = _ext._pad(u.shape[2:], 1)
    elems = _ext._scratch_elems(_ext._lib.lago_field_energy_scratch_elems, k, dim, N, C, *n)
    E = torch.empty((N,), dtype=u.dtype, device=u.device)
    scratch = torch.empty((elems,), dtype=u.dtype, device=u.device)
    _ext._call("lago_field_energy", u, _ext._ptr(E), _ext._ptr(u), _ext._ptr(scratch), elems, k, dim, N, C, *n, (ctypes.c_double * dim)(*sp))
    return E


def _operator(u, kind, spacing, scale):
    """scale[n] (A u)[n] by lago_field_energy_operator (csrc/energy.hip: energy_operator_kernel)."""
    k, dim, sp = _check(u, kind, spacing, "energy_operator", scale)
    out = torch.empty_like(u)
    if u.numel() == 0:
        return out
    _ext._call("lago_field_energy_operator", u, _ext._ptr(out), _ext._ptr(u), _ext._ptr(scale), k, dim, u.size(0), u.size(1), *_ext._pad(u.shape[2:], 1),
               (ctypes.c_double * dim)(*sp))
    return out


class EnergyOperatorFunction(torch.autograd.Function):
    """(u, scale) -> scale[n] (A u)[n].  A is linear and symmetric, so the backward with respect to u is the same
    function applied to the incoming gradient with the same scale -- differentiable to any order -- and the one with
    respect to scale, computed only when asked for, is the per-item dot product <g, A u>."""

    @staticmethod
    def forward(ctx, u, kind, spacing, scale):
        ctx.kind, ctx.spacing = kind, spacing
        ctx.save_for_backward(u, scale)
        return _operator(u, kind, spacing, scale)

    @staticmethod
    def backward(ctx, gradout):
        u, scale = ctx.saved_tensors
        d_u = d_scale = None
        if ctx.needs_input_grad[0]:   # no kernel runs for a gradient nobody needs
            d_u = EnergyOperatorFunction.apply(gradout.contiguous(), ctx.kind, ctx.spacing, scale)
        if scale is not None and ctx.needs_input_grad[3]:
            Au = EnergyOperatorFunction.apply(u, ctx.kind, ctx.spacing, None)
            d_scale = (gradout * Au).flatten(1).sum(1)
        return d_u, None, None, d_scale


class FieldEnergyFunction(torch.autograd.Function):
    """u -> E (N,).  The backward is the differentiable operator function, dE_n/du = (2 g_n / V) A u, the factor handed
    to the kernel as a device vector: the energies are differentiable twice."""

    @staticmethod
    def forward(ctx, u, kind, spacing):
        ctx.kind, ctx.spacing = kind, spacing
        ctx.save_for_backward(u)
        return _energy(u, kind, spacing)

    @staticmethod
    def backward(ctx, gradout):
        if not ctx.needs_input_grad[0]:   # no kernel runs for a gradient nobody needs
            return None, None, None
        u, = ctx.saved_tensors
        V = max(1, math.prod(u.shape[2:]))
        return EnergyOperatorFunction.apply(u, ctx.kind, ctx.spacing, (gradout * (2.0 / V)).contiguous()), None, None


def field_energy(u, kind, spacing=1.0):
    """E (N,): the energy of kind "diffusion" or "bending" (module docstring) of every item of u (N, C, *sp).

    One streaming read of u: workgroups own voxel tiles staged in on-chip memory with their halo, every lane adds its
    voxels' terms, and a second small kernel adds the tiles' partial sums in double in a fixed order.  No atomics: the
    bits repeat from call to call.  float32 energies are within about 1e-6 of their value.

    Differentiable in u twice (the backward is `energy_operator` with scale 2 g / V, itself differentiable).

    RuntimeError for dtypes, shapes, spacings or kinds that do not fit, non-contiguous or CPU tensors; TypeError for
    anything that is not a tensor."""
    return FieldEnergyFunction.apply(u, kind, spacing)


def diffusion_energy(u, spacing=1.0):
    """E (N,): the mean squared forward difference of u (N, C, *sp), summed over channels and axes -- `field_energy`
    of kind "diffusion"."""
    return FieldEnergyFunction.apply(u, "diffusion", spacing)


def bending_energy(u, spacing=1.0):
    """E (N,): the mean squared second derivatives of u (N, C, *sp), mixed ones twice, summed over channels --
    `field_energy` of kind "bending".  Exactly 0 for a field that is affine in the voxel index.  For an FFD,
    bending_energy(ffd_expand(c, shape, s)) penalises the dense field and its gradient reaches the lattice through
    `ffd_restrict`."""
    return FieldEnergyFunction.apply(u, "bending", spacing)


def energy_operator(u, kind, spacing=1.0, scale=None):
    """out (N, C, *sp) = scale[n] (A u)[n], A the operator of E = <u, A u> / V (module docstring): what the backward of
    the energies runs, as a public function (dE/du = (2/V) A u; also the matrix-free operator of a Gauss-Newton or
    conjugate-gradient step).  `scale`: None for 1, or a tensor (N,) of u's dtype on its device.

    One load and one store per element; plain stores: the bits repeat from call to call.  A float32 value is within
    K 2^-24 |scale| sum |A| |u| of the exact one, K = 13 for bending and 8 for diffusion.

    Differentiable in u to any order and in scale.  Errors as for `field_energy`."""
    return EnergyOperatorFunction.apply(u, kind, spacing, scale)
