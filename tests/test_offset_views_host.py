"""CPU: tests/offset_views.py itself, so that the guard of tests/test_gpu_alignment.py cannot pass vacuously: the
misalignment arithmetic, the values, and that `margins_intact` sees one planted element on either side of the view and
nothing else."""
import pytest
import torch

from offset_views import OFFSETS, PAD, margins_intact, offset_view, poison_of, poisoned

DTYPES = [torch.float32, torch.float64, torch.int32, torch.int16, torch.int64, torch.uint8]


def _values(dtype, shape=(2, 3, 5, 7)):
    g = torch.Generator().manual_seed(3)
    if dtype.is_floating_point:
        return torch.randn(shape, dtype=dtype, generator=g)
    return torch.randint(0, 6, shape, dtype=dtype, generator=g)


def _pad(dtype):
    return max(PAD, 16 // torch.empty((), dtype=dtype).element_size())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("off", (0,) + OFFSETS)
def test_view_is_where_it_says_and_holds_the_values(dtype, off):
    t = _values(dtype)
    pad = _pad(dtype)
    view, buf = offset_view(t, off, pad=pad)
    size = t.element_size()
    assert buf.dim() == 1 and buf.numel() == t.numel() + 2 * pad and buf.dtype == t.dtype
    assert buf.data_ptr() % 64 == 0
    assert view.is_contiguous() and view.shape == t.shape
    assert view.data_ptr() == buf.data_ptr() + (pad + off) * size
    assert view.data_ptr() % 16 == (off * size) % 16
    if size >= 4:
        assert (view.data_ptr() % 16 == 0) == (off * size % 16 == 0)
    if dtype == torch.float64:   # 1 and 3 break the 16-byte alignment, 2 keeps it and breaks the 32-byte one
        assert view.data_ptr() % 32 == {0: 0, 1: 8, 2: 16, 3: 24}[off]
    assert torch.equal(view, t)
    assert view.data_ptr() != t.data_ptr()            # a copy: writes to the view leave t alone
    assert margins_intact(buf, view) == []
    assert poisoned(view) == 0
    # the view shares the buffer's storage: what a callee writes through it lands between the margins
    view.zero_()
    assert margins_intact(buf, view) == [] and not buf[pad + off:pad + off + t.numel()].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_float_poison_is_a_quiet_nan_with_exact_bits(dtype):
    t = _values(dtype)
    view, buf = offset_view(t, 1)
    idt, bits = poison_of(dtype)
    margin = torch.cat([buf[:PAD + 1], buf[PAD + 1 + t.numel():]])
    assert torch.isnan(margin).all() and margin.numel() == 2 * PAD
    assert (margin.view(idt) == bits).all()
    quiet = 1 << (22 if dtype == torch.float32 else 51)
    assert bits & quiet and bits & (quiet - 1)        # quiet bit set, payload not empty
    assert poisoned(buf) == 2 * PAD
    assert not torch.isnan(view).any()


@pytest.mark.parametrize("dtype", [torch.int32, torch.uint8, torch.int16, torch.int64], ids=str)
def test_label_poison_is_outside_every_label_range(dtype):
    _, p = poison_of(dtype)
    info = torch.iinfo(dtype)
    assert info.min <= p <= info.max and p not in (0, -1, 255)
    assert p >= 4096 or dtype == torch.uint8          # LAGO_LABELS_MAX; uint8 cases use K well below 0xEE
    view, buf = offset_view(_values(dtype), 2, pad=_pad(dtype))
    assert poisoned(buf) == 2 * _pad(dtype) and poisoned(view) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("off", (0,) + OFFSETS)
def test_margins_intact_reports_a_planted_write(dtype, off):
    t = _values(dtype, (3, 11))
    pad = _pad(dtype)
    first, last = pad + off, pad + off + t.numel() - 1
    for where in (first - 1, last + 1, 0, t.numel() + 2 * pad - 1):
        view, buf = offset_view(t, off, pad=pad)
        buf[where] = 1
        assert margins_intact(buf, view) == [where]
    view, buf = offset_view(t, off, pad=pad)
    buf[first - 1] = 1
    buf[last + 1] = 2
    assert margins_intact(buf, view) == [first - 1, last + 1]
    # writes inside the view, its first and last element included, are the callee's business
    view, buf = offset_view(t, off, pad=pad)
    buf[first] = 1
    buf[last] = 1
    assert margins_intact(buf, view) == []


def test_a_float_margin_rewritten_with_another_nan_is_reported():
    """The comparison is on bits: a NaN of another payload (what an arithmetic result would be) is a change."""
    t = _values(torch.float32, (4, 5))
    view, buf = offset_view(t, 3)
    buf[PAD + 2] = float("nan")
    assert margins_intact(buf, view) == [PAD + 2]


def test_unpoisoned_margins_and_bad_arguments():
    t = _values(torch.float32, (4, 5))
    view, buf = offset_view(t, 1, poison=False)
    assert not buf[:PAD + 1].any() and not buf[PAD + 1 + t.numel():].any() and torch.equal(view, t)
    with pytest.raises(AssertionError):
        offset_view(t, PAD + 1)
    with pytest.raises(AssertionError):
        offset_view(_values(torch.uint8), 1)          # 8 bytes of margin would shift every offset by 8
