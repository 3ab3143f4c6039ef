"""Test-side reference for invert_displacement (numpy, no GPU), built from the CPU oracle's interp routines, which
are pinned to the reference's own code:

  * forward(u, iters): v = -u, then `iters` times v = -oracle interp_forward(u, v, 1.0);
  * G(u, v)[c][a] = (d_a u_c)(x + v(x)): oracle interp_backward with a one-hot grad_out on channel c and need_u -- its
    d_u[a] is fma(gradient_a, 1, 0), the rounded gradient of the interpolant itself;
  * lam(go, u, v) = -(I + G)^-T go per voxel, a float64 numpy solve;
  * d_u(go, u, v): that lam splatted at x + v by oracle interp_backward(need_I=True).

`field` makes the inputs of the tests: an analytic smooth field rescaled so that a computed bound on the Lipschitz
constant of its multilinear interpolant is 0.5, i.e. the fixed-point map is a contraction at rate 0.5 at the worst.

`np_interp` / `np_forward` are an independent pure-numpy restatement of the clamped multilinear interpolation that the
CPU suite holds the above against.
"""
import itertools

import numpy as np

from oracle import lago_oracle as orc


def forward(u, iters):
    u = np.ascontiguousarray(u)
    v = -u
    for _ in range(iters):
        v = -orc.interp_forward(u, v, 1.0)
    return v


def G(u, v):
    """G[c][a] as a list of lists of (N, *sp) arrays in u's dtype."""
    u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
    d = u.shape[1]
    assert d == u.ndim - 2 and d in (2, 3) and v.shape == u.shape, (u.shape, v.shape)
    out = []
    for c in range(d):
        go = np.zeros_like(u)
        go[:, c] = 1
        _, du = orc.interp_backward(go, u, v, 1.0, False, True)
        out.append([du[:, a] for a in range(d)])
    return out


def lam(go, u, v):
    """float64 (N, d, *sp): -(I + G)^-T go."""
    g = G(u, v)
    d = len(g)
    M = np.stack([np.stack([g[c][a].astype(np.float64) for a in range(d)], axis=-1) for c in range(d)], axis=-2)
    M = M + np.eye(d)                                            # (N, *sp, c, a)
    rhs = np.moveaxis(np.asarray(go, dtype=np.float64), 1, -1)[..., None]
    sol = np.linalg.solve(np.swapaxes(M, -1, -2), rhs)[..., 0]   # M^T lam = go
    return np.ascontiguousarray(-np.moveaxis(sol, -1, 1))


def min_det(u, v):
    g = G(u, v)
    d = len(g)
    M = np.stack([np.stack([g[c][a].astype(np.float64) for a in range(d)], axis=-1) for c in range(d)], axis=-2)
    return float(np.linalg.det(M + np.eye(d)).min())


def d_u(go, u, v):
    """d_u like u: the splat of lam at x + v."""
    u = np.ascontiguousarray(u)
    lm = lam(go, u, v).astype(u.dtype)
    return orc.interp_backward(lm, u, np.ascontiguousarray(v), 1.0, True, False)[0]


# ---- test fields

def lipschitz_bound(u):
    """sqrt(sum_{c,a} (max |edge difference of u_c along a|)^2), in float64.  Inside a cell d_a u_c of the multilinear
    interpolant is a convex combination of the cell's edge differences along a, so the Frobenius norm of its Jacobian
    -- hence its Lipschitz constant -- is at most this; clamping at the border composes with a projection (Lipschitz 1)
    and does not raise it."""
    u = np.asarray(u, dtype=np.float64)
    tot = 0.0
    for c in range(u.shape[1]):
        for a in range(u.shape[1]):
            dif = np.diff(u[:, c], axis=1 + a)
            tot += float(np.abs(dif).max()) ** 2 if dif.size else 0.0
    return float(np.sqrt(tot))


def field(sp, nn, dtype, L=0.5):
    """(nn, d, *sp) of `dtype`: u_c = sin(2 pi (x_c + .5) / n_c + .7 c + .4 n + .2) cos(2 pi (x_{c+1} + .25) / n_{c+1} + .3),
    rescaled to lipschitz_bound == L (the bound is homogeneous).  float32: scaled a hair further down (1e-5) so that
    rounding the values to float32 cannot lift the bound of the array the test uses above L.  (The phase .2 keeps the
    sine's zeros off the grid points: where u_c vanishes, x + v sits exactly on a cell face, a kink of the interpolant,
    and a one-sided derivative is all a gradient check could find there.)"""
    d = len(sp)
    x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sp], indexing="ij")
    u = np.empty((nn, d) + tuple(sp))
    for n in range(nn):
        for c in range(d):
            e = (c + 1) % d
            u[n, c] = (np.sin(2 * np.pi * (x[c] + .5) / sp[c] + .7 * c + .4 * n + .2)
                       * np.cos(2 * np.pi * (x[e] + .25) / sp[e] + .3))
    dtype = np.dtype(dtype)
    u *= L / lipschitz_bound(u) * (1 - 1e-5 if dtype == np.float32 else 1.0)
    return np.ascontiguousarray(u.astype(dtype))


# ---- the independent restatement (numpy, any float dtype)

def np_interp(I, u):
    """I(x + u(x)), multilinear, floor / floor + 1 corners each clamped into the grid.  I: (N, C, *sp), u: (N, d, *sp)."""
    I, u = np.asarray(I), np.asarray(u)
    d = u.shape[1]
    sp = u.shape[2:]
    x = np.meshgrid(*[np.arange(n, dtype=u.dtype) for n in sp], indexing="ij")
    out = np.zeros(I.shape, dtype=I.dtype)
    for n in range(u.shape[0]):
        p = [x[a] + u[n, a] for a in range(d)]
        fl = [np.floor(q) for q in p]
        t = [q - f for q, f in zip(p, fl)]
        fl = [f.astype(np.int64) for f in fl]
        for corner in itertools.product((0, 1), repeat=d):
            w = np.ones(sp, dtype=u.dtype)
            idx = []
            for a, o in enumerate(corner):
                w = w * (t[a] if o else 1 - t[a])
                idx.append(np.clip(fl[a] + o, 0, sp[a] - 1))
            out[n] += w * I[n][(slice(None),) + tuple(idx)]
    return out


def np_forward(u, iters):
    v = -np.asarray(u)
    for _ in range(iters):
        v = -np_interp(u, v)
    return v
