"""Contiguous views that start a few elements past a 16-byte boundary, inside a buffer with poisoned margins.

The library takes raw data pointers of any contiguous tensor (lagomorph_ext._ptr), so a field carved out of a packed
parameter buffer, `flat[1:1 + n].view(shape)`, reaches the kernels with a base that is element-aligned and nothing more.
`offset_view` builds such a view of given values; the margins on both sides hold a poison, so that

 * a store that rounds its address down, or a tail that runs past the end, changes margin bits (`margins_intact`), and
 * a load that reaches into a margin and then into an output turns up there: a NaN for floating types, POISON_LABEL for
   label maps.

No GPU is needed to import this module; tests/test_offset_views_host.py holds it against CPU tensors."""
import torch

PAD = 8
# quiet NaNs with a payload one recognises in a dump; written through an integer view, so that no conversion or
# NaN canonicalisation touches the bits
_FLOAT_POISON = {torch.float32: (torch.int32, 0x7FC0BEEF), torch.float64: (torch.int64, 0x7FF80000DEADBEEF)}
# labels: above LAGO_LABELS_MAX (4096) and positive, hence outside every [0, K) the tests use, and unlike the values
# callers use to mark voxels to be left out (0, -1, 255)
_INT_POISON = {torch.uint8: 0xEE, torch.int16: 0x5EED, torch.int32: 0x5EEDBEEF, torch.int64: 0x5EEDBEEF5EEDBEEF}
OFFSETS = (1, 2, 3)    # elements; 0 is the control and goes through the same helper


def poison_of(dtype):
    """(integer dtype the bits are compared in, the poison as a Python int)."""
    if dtype in _FLOAT_POISON:
        return _FLOAT_POISON[dtype]
    return dtype, _INT_POISON[dtype]


def _bits(t):
    return t.view(poison_of(t.dtype)[0])


def offset_view(t, off, pad=PAD, poison=True):
    """(view, buf): `buf` a flat buffer of t.numel() + 2 pad elements like t whose storage starts on a 64-byte boundary,
    `view` the contiguous view of t's shape that starts at element pad + off and holds t's values.  0 <= off <= pad.  The
    elements of `buf` outside the view hold the poison of t's dtype (poison=False: zeros)."""
    assert 0 <= off <= pad, (off, pad)
    assert (pad * t.element_size()) % 16 == 0, "the leading margin must be whole 16-byte units (uint8: pad=16)"
    n = t.numel()
    buf = torch.zeros(n + 2 * pad, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 64 == 0, "the allocator is expected to return 64-byte aligned storage"
    if poison:
        _bits(buf).fill_(poison_of(t.dtype)[1])
    view = buf[pad + off:pad + off + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.shape == t.shape
    assert view.data_ptr() % 16 == (off * t.element_size()) % 16
    return view, buf


def margins_intact(buf, view):
    """Indices into `buf` of margin elements whose bits are no longer the poison (an empty list: intact)."""
    start = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    assert 0 <= start and start + view.numel() <= buf.numel()
    changed = _bits(buf) != poison_of(buf.dtype)[1]
    changed[start:start + view.numel()] = False
    return changed.nonzero().flatten().tolist()


def poisoned(t):
    """How many elements of t hold the poison of its dtype (bit for bit)."""
    return int((_bits(t.contiguous()) == poison_of(t.dtype)[1]).sum())
