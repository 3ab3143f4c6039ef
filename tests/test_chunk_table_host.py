"""Host check of the chunked-table frame's arithmetic (no GPU needed).

lagomorph_amd/csrc/chunk_table.hpp holds, once, how the joint histogram (csrc/mi.hip) and the overlap counts
(csrc/labels.hip) split a row of nvox elements into chunks and a chunk into a scalar head, vectors and a scalar tail.
tests/native/chunk_table_emul.cpp runs the header's host part with a plain C++17 compiler (and once more built with
-fsanitize=address,undefined) over a grid of inputs; here the answers are held against

  * the formulas of the two files as they stood before the header, restated in Python integers: mi_split and
    mi_tables_wanted of mi.hip, the block in label_overlap_impl and overlap_chunks_wanted of labels.hip;
  * what the kernels rely on: the chunk is a multiple of four, the chunks cover the row, none is empty, no more chunks
    than the caller's scratch holds, and the slab stays under 8 MB unless a row has one chunk;
  * for the walk: the three parts add up to n, every vector starts on a vector boundary, and pointers that are
    misaligned differently get no vector at all.

The two scratch queries of the C ABI answer the same restatement on the same grid."""
import native_build

SLAB = 8 << 20
MI_CHUNK, LABELS_CHUNK = 4096, 16384   # kMiChunkMin of mi.hip, LAGO_LABELS_CHUNK of labels.hip
NVOX = [*range(0, 71), *range(4095, 4101), *range(16383, 16391), 54120, 1 << 30]
ROWS = [1, 2, 3, 8, 1000, (1 << 31) - 1]
BINS = [4, 5, 32, 45, 46, 64]
LABELS = [1, 200, 1365, 1366, 2730, 4096]
TABLES = [(B * B * 8, MI_CHUNK) for B in BINS] + [(K * 3 * 4, LABELS_CHUNK) for K in LABELS]   # (bytes, chunk_min)
CAPS = [1, 2, 3, -1, -2]               # -1: what is wanted, -2: five more


def ceil_div(a, b):
    return -(-a // b)


def wanted_before(table_bytes, rows, nvox, chunk_min):
    """mi_tables_wanted / overlap_chunks_wanted."""
    by_size = ceil_div(nvox, chunk_min)
    cap = SLAB // table_bytes // max(rows, 1)
    return max(min(by_size, cap), 1)


def mi_split_before(nvox, want, least):
    """mi_split (reached with nvox > 0 only)."""
    c = max(min(ceil_div(nvox, least), want), 1)
    per = (ceil_div(nvox, c) + 3) // 4 * 4
    return per, ceil_div(nvox, per)


def overlap_split_before(table_bytes, rows, nvox, scratch_chunks):
    """The block in label_overlap_impl."""
    c = min(wanted_before(table_bytes, rows, nvox, LABELS_CHUNK), scratch_chunks)
    per = (ceil_div(nvox, c) + 3) // 4 * 4
    return per, (ceil_div(nvox, per) if per else 1)


def _build(tmp_path, name, extra=()):
    return native_build.build(tmp_path, "chunk_table_emul.cpp", "-O1", fp_contract_off=False, extra=extra, name=name)


def _cases():
    split = [(tb, rows, nvox, cm, cap) for tb, cm in TABLES for rows in ROWS for nvox in NVOX for cap in CAPS]
    walk = [(vw, n, same, mis) for vw in (2, 4) for n in range(41) for same in (0, 1) for mis in range(vw)]
    return split, walk


def _run(exe):
    split, walk = _cases()
    text = "".join("C %d %d %d %d %d\n" % c for c in split) + "".join("W %d %d %d %d\n" % c for c in walk)
    r = native_build.run(exe, stdin=text, quiet=True)
    out = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(out) == len(split) + len(walk)
    return split, out[:len(split)], walk, out[len(split):]


def _check(split, got_split, walk, got_walk):
    two_chunks = 0
    for (tb, rows, nvox, cm, cap_code), (want, cap, chunks, chunk) in zip(split, got_split):
        what = (tb, rows, nvox, cm, cap_code)
        assert want == wanted_before(tb, rows, nvox, cm), what
        assert cap == {-1: want, -2: want + 5}.get(cap_code, cap_code), what
        # the formulas before the header
        if cm == LABELS_CHUNK:
            assert (chunk, chunks) == overlap_split_before(tb, rows, nvox, cap), what
        if nvox > 0:
            assert (chunk, chunks) == mi_split_before(nvox, min(want, cap), cm), what
        else:
            assert (chunk, chunks) == (0, 1), what
        # what the kernels rely on
        assert chunk % 4 == 0 and chunks * chunk >= nvox and 1 <= chunks <= cap, what
        if nvox > 0:
            assert (chunks - 1) * chunk < nvox, what
        assert rows * chunks * tb <= SLAB or chunks == 1, what
        two_chunks += chunks >= 2
    assert two_chunks > 1000   # the grid does split rows
    vectors = 0
    for (vw, n, same, mis), (head, nvec, tail) in zip(walk, got_walk):
        what = (vw, n, same, mis)
        assert head == (min((vw - mis) % vw, n) if same else n) and nvec == (n - head) // vw and tail == head + nvec * vw, what
        assert head + vw * nvec + (n - tail) == n and 0 <= head <= tail <= n, what
        if same:
            assert all((mis + head + v * vw) % vw == 0 for v in range(nvec)), what
            assert n - tail < vw, what
        else:
            assert head == n and nvec == 0, what
        vectors += nvec
    assert vectors > 500


@native_build.needs_cxx
def test_header_arithmetic_equals_the_formulas_it_replaced(tmp_path):
    _check(*_run(_build(tmp_path, "chunk_table_emul")))


@native_build.needs_cxx
def test_header_arithmetic_under_the_sanitizers(tmp_path):
    """The same stand-alone host program with AddressSanitizer and UndefinedBehaviorSanitizer: no division by zero for an
    empty row, no overflow at 2^31 - 1 rows of 2^30 voxels."""
    _check(*_run(_build(tmp_path, "chunk_table_emul_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))))


def test_scratch_queries_equal_the_formulas_they_replaced():
    from lagomorph_amd import lagomorph_ext as ext

    mi, lab = ext._lib.lago_mi_scratch_tables, ext._lib.lago_label_overlap_scratch_chunks
    for rows in [0] + ROWS:
        for nvox in NVOX:
            for B in BINS:
                assert mi(B, rows, nvox) == wanted_before(B * B * 8, rows, nvox, MI_CHUNK), (B, rows, nvox)
            for K in LABELS:
                assert lab(K, rows, nvox) == wanted_before(K * 12, rows, nvox, LABELS_CHUNK), (K, rows, nvox)
    # arguments the entry points reject: one table
    for bad in ((3, 8, 1 << 20), (65, 8, 1 << 20), (32, -1, 1 << 20), (32, 8, -1), (32, 8, (1 << 30) + 1)):
        assert mi(*bad) == 1, bad
    assert mi(32, 8, 1 << 20) > 1
    for bad in ((0, 8, 1 << 20), (4097, 8, 1 << 20), (5, -1, 1 << 20), (5, 8, -1), (5, 8, (1 << 30) + 1)):
        assert lab(*bad) == 1, bad
    assert lab(5, 8, 1 << 20) > 1
