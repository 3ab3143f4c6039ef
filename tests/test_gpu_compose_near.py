"""compose with the near-identity hint (csrc/fused.hip: compose3_near_kernel -- the window on the tile itself, two
windows in flight) against the two kernels it must agree with bit for bit: the pair-gather kernel
(`set_gather_window(0)`) and the translated-window kernel (the same call without the hint).  The hint selects a kernel,
never a value, so every case is `torch.equal`, whatever the field does to the promise "|ds u| < 1 voxel".

Shapes: the smallest the window kernels accept (nz % 4 == 0, >= 32768 voxels, >= 85 % tile fill): whole 8 x 16 x 32
tiles, a partial tile in x (36: 90 % fill), and more than one tile along y and z."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DS, DT = -0.1, 1.0
SHAPES = [(2, 3, 32, 32, 32), (2, 3, 36, 32, 32), (1, 3, 32, 48, 64)]


@pytest.fixture(scope="module")
def ext():
    import lagomorph_amd

    return lagomorph_amd.lagomorph_ext


@contextlib.contextmanager
def tuned(ext, **fields):
    saved = ext.get_tuning()
    ext.tune(**fields)
    try:
        yield
    finally:
        ext.tune(**{k: saved[k] for k in fields})


def _smooth(sh, g, amp):
    """a smooth field with max |.| = amp"""
    f = torch.randn(sh, device="cuda", generator=g)
    for _ in range(2):
        f = torch.nn.functional.avg_pool3d(f, 7, stride=1, padding=3, count_include_pad=False)
    return (f * (amp / f.abs().max())).contiguous()


def _offsets_to_u(off):
    return (off * (1.0 / DS)).contiguous()   # the sample of voxel x lies at x + DS * u; 1 / DS = -10 exactly


def _const(axis, value):
    def make(sh, g):
        off = torch.zeros(sh, device="cuda")
        off[:, axis] = value
        return _offsets_to_u(off)
    return make


def _block(sh, g):
    u = _smooth(sh, g, 0.3 / abs(DS))
    u[:, :, 9:13, 10:14, 17:21] = 3.0 / DS   # one 4^3 block three voxels away, inside a tile: strays among window samples
    return u.contiguous()


def _outward(sh, g):
    """every sample points away from the volume's centre, 0.4 to 1.8 voxels: clamped rows on all six faces (f_hi / c_lo
    in z), and corners one cell beyond the small window"""
    off = torch.empty(sh, device="cuda")
    for a in range(3):
        n = sh[2 + a]
        sign = torch.where(torch.arange(n, device="cuda") < n / 2, -1.0, 1.0)
        shape = [1, 1, 1]
        shape[a] = n
        off[:, a] = sign.view(shape)
    mag = 0.4 + 1.4 * torch.rand(sh, device="cuda", generator=g)
    return _offsets_to_u(off * mag)


FIELDS = {
    "zero": lambda sh, g: torch.zeros(sh, device="cuda"),
    "euler_step": lambda sh, g: _smooth(sh, g, 0.6 / abs(DS)),        # |ds u| <= 0.6: what the shoot does
    "far": lambda sh, g: _smooth(sh, g, 2.5 / abs(DS)),               # |ds u| up to 2.5: tiles that leave the small window
    "block": _block,
    "outward": _outward,
}
for _axis in range(3):
    for _value in (1.0, -1.0, 0.999, -0.999):                         # floor boundaries of the one-voxel promise
        FIELDS[f"const_{'xyz'[_axis]}_{_value:+g}"] = _const(_axis, _value)


@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("sh", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_near_identity_compose_has_the_bits_of_both_other_kernels(ext, sh, field):
    g = torch.Generator(device="cuda").manual_seed(100 * SHAPES.index(sh) + list(FIELDS).index(field))
    u = FIELDS[field](sh, g)
    v = torch.randn(sh, device="cuda", generator=g)
    with tuned(ext, compose_near=1):
        before = ext.path_launches()
        near = ext.compose(u, v, DS, DT, near_identity=True)
        after = ext.path_launches()
        assert after["gather_window_near"] == before["gather_window_near"] + 1 and after["gather_window"] == before["gather_window"]
        before = after
        window = ext.compose(u, v, DS, DT)
        after = ext.path_launches()
        assert after["gather_window"] == before["gather_window"] + 1
        with tuned(ext, gather_window=0):
            before = ext.path_launches()
            pair = ext.compose(u, v, DS, DT, near_identity=True)
            after = ext.path_launches()
            assert after["vector_gather"] == before["vector_gather"] + 1 and after["gather_window_near"] == before["gather_window_near"]
    assert torch.equal(window, pair), "the two existing kernels disagree: not this test's subject"
    assert torch.equal(near, pair), f"near-identity compose != pair gathers ({(near != pair).sum().item()} values)"
    assert torch.equal(near, window)


def test_exact_unit_offsets_are_exact():
    """the floor-boundary fields mean what they say: in float32, fl(fl(-0.1) * -10) == 1 exactly, so a sample of the
    +-1.0 fields sits ON the neighbouring voxel (the kernels multiply by ds rounded to float32)"""
    assert float(torch.tensor(DS, dtype=torch.float32) * torch.tensor(1.0 / DS, dtype=torch.float32)) == 1.0


def _delta(ext, f):
    before = ext.path_launches()
    f()
    torch.cuda.synchronize()
    after = ext.path_launches()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def test_the_hint_and_the_knob_choose_the_kernel(ext):
    g = torch.Generator(device="cuda").manual_seed(5)
    sh = (1, 3, 32, 32, 32)
    u, v = torch.randn(sh, device="cuda", generator=g), torch.randn(sh, device="cuda", generator=g)
    assert "compose_near" in ext.get_tuning()
    with tuned(ext, compose_near=1):
        assert _delta(ext, lambda: ext.compose(u, v, DS, DT, near_identity=True)) == {"gather_window_near": 1}
        assert _delta(ext, lambda: ext.compose(u, v, DS, DT)) == {"gather_window": 1}
        with tuned(ext, gather_window=0):     # still forces the pair gathers
            assert _delta(ext, lambda: ext.compose(u, v, DS, DT, near_identity=True)) == {"vector_gather": 1}
        # shapes and types the window kernels do not take keep their kernels, hint or not
        assert _delta(ext, lambda: ext.compose(u.double(), v.double(), DS, DT, near_identity=True)) == {"vector_gather": 1}
        small = torch.randn((1, 3, 8, 16, 32), device="cuda", generator=g)
        assert "gather_window_near" not in _delta(ext, lambda: ext.compose(small, small, DS, DT, near_identity=True))
    with tuned(ext, compose_near=0):
        assert _delta(ext, lambda: ext.compose(u, v, DS, DT, near_identity=True)) == {"gather_window": 1}


def test_expmap_has_the_same_bits_with_the_near_identity_arm_on_and_off(ext):
    import lagomorph_amd as lm

    g = torch.Generator(device="cuda").manual_seed(77)
    sh = (2, 3, 32, 32, 32)
    metric = lm.FluidMetric([0.1, 0.0, 0.01])
    with torch.no_grad():
        m0 = _smooth(sh, g, 1.0)
        m0 = (m0 * (3.0 / metric.sharp(m0).abs().max())).contiguous()   # a 3-voxel shoot in three steps: one voxel a step
        with tuned(ext, compose_near=1):
            took = _delta(ext, lambda: lm.expmap(metric, m0, num_steps=3))
            on = lm.expmap(metric, m0, num_steps=3)
        with tuned(ext, compose_near=0):
            took_off = _delta(ext, lambda: lm.expmap(metric, m0, num_steps=3))
            off = lm.expmap(metric, m0, num_steps=3)
    # the general steps (two per part of the shoot; the first step is closed-form) change kernels, and nothing else does
    assert took.get("gather_window_near", 0) >= 2 and "gather_window" not in took, took
    assert "gather_window_near" not in took_off and took_off.get("gather_window") == took["gather_window_near"], took_off
    assert {k: n for k, n in took.items() if k != "gather_window_near"} == {k: n for k, n in took_off.items() if k != "gather_window"}
    assert torch.equal(on, off)
