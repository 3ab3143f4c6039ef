"""Test-side reference for jacobian_determinant (numpy, no GPU), built from the CPU oracle's
jacobian_times_vectorfield routines, which are pinned to the reference's own code:

  * J[c][a] = oracle jtv_forward(u, e_a, displacement, transpose=False)[:, c] with e_a the constant unit field; the
    contraction with a unit vector is exact, so these are the rounded clamped differences (plus the 1) themselves;
  * forward: the determinant expression of include/lagomorph_hip.h in u's dtype, every product and sum rounded on its own;
  * backward: the cofactors in numpy, then oracle jtv_adjoint_forward(grad_out, C[c][:]) per component c, which is
    sum_a D_a^T (grad_out * C[c][a]).

`torch_forward` / `torch_backward` are an independent pure-torch restatement (index-clamped differences by
index_select, the same determinant expression, autograd for the gradient) that the CPU suite holds the above against.
"""
import numpy as np

from oracle import lago_oracle as orc


def jacobian(u, displacement):
    """J[c][a] as a list of lists of (N, *sp) arrays."""
    u = np.ascontiguousarray(u)
    d = u.shape[1]
    assert d == u.ndim - 2 and d in (2, 3), u.shape
    cols = []
    for a in range(d):
        e = np.zeros_like(u)
        e[:, a] = 1
        cols.append(orc.jacobian_times_vectorfield_forward(u, e, bool(displacement), False))
    return [[cols[a][:, c] for a in range(d)] for c in range(d)]


def det(J):
    if len(J) == 2:
        return J[0][0] * J[1][1] - J[0][1] * J[1][0]
    return ((J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]))
            + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))


def cofactors(J):
    """C[c][a] = d det / d J[c][a]."""
    d = len(J)
    if d == 2:
        return [[J[1][1], -J[1][0]], [-J[0][1], J[0][0]]]
    return [[J[(c + 1) % 3][(a + 1) % 3] * J[(c + 2) % 3][(a + 2) % 3]
             - J[(c + 1) % 3][(a + 2) % 3] * J[(c + 2) % 3][(a + 1) % 3] for a in range(3)] for c in range(3)]


def forward(u, displacement=True):
    """(N, 1, *sp), in u's dtype."""
    out = det(jacobian(u, displacement))
    assert out.dtype == np.asarray(u).dtype
    return np.ascontiguousarray(out[:, None])


def backward(grad_out, u, displacement=True):
    """d_u like u for grad_out of shape (N, 1, *sp)."""
    u = np.ascontiguousarray(u)
    grad_out = np.ascontiguousarray(grad_out, dtype=u.dtype)
    assert grad_out.shape == (u.shape[0], 1) + u.shape[2:], (grad_out.shape, u.shape)
    C = cofactors(jacobian(u, displacement))
    d_u = np.empty_like(u)
    for c in range(u.shape[1]):
        w = np.ascontiguousarray(np.stack(C[c], axis=1))
        d_u[:, c] = orc.jacobian_times_vectorfield_adjoint_forward(grad_out, w)[:, 0]
    return d_u


# ---- the independent restatement (torch on the CPU)

def _torch_det(u, displacement):
    import torch

    d = u.shape[1]
    J = [[None] * d for _ in range(d)]
    for a in range(d):
        ax = 2 + a
        n = u.shape[ax]
        idx = torch.arange(n)
        up = torch.index_select(u, ax, torch.clamp(idx + 1, max=n - 1))
        um = torch.index_select(u, ax, torch.clamp(idx - 1, min=0))
        g = 0.5 * (up - um)
        for c in range(d):
            J[c][a] = g[:, c] + 1.0 if (displacement and a == c) else g[:, c]
    return det(J)[:, None]


def torch_forward(u, displacement=True):
    import torch

    return _torch_det(torch.from_numpy(np.ascontiguousarray(u)), displacement).numpy()


def torch_backward(grad_out, u, displacement=True):
    import torch

    ut = torch.from_numpy(np.ascontiguousarray(u)).requires_grad_(True)
    _torch_det(ut, displacement).backward(torch.from_numpy(np.ascontiguousarray(grad_out)))
    return ut.grad.numpy()
