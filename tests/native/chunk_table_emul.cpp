// Host check of lagomorph_amd/csrc/chunk_table.hpp (tests/test_chunk_table_host.py): the first part of the header --
// the number of chunks wanted, the split of a row and the head / vector / tail split of a chunk -- built by a plain
// C++17 compiler, no HIP.  Reads cases from stdin, one a line, and answers each on stdout:
//   C table_bytes rows nvox chunk_min cap   ->  wanted cap chunks chunk   (cap -1: what is wanted, -2: five more)
//   W vw n same mis                         ->  head nvec tail
#include <inttypes.h>
#include <stdio.h>

#include "../../lagomorph_amd/csrc/chunk_table.hpp"

using namespace lago;

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'C') {
            int64_t table_bytes, rows, nvox, chunk_min, cap;
            if (scanf("%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64, &table_bytes, &rows, &nvox, &chunk_min, &cap) != 5) return 2;
            const int64_t want = chunks_wanted(table_bytes, rows, nvox, chunk_min, kSlabBytes);
            if (cap < 0) cap = cap == -1 ? want : want + 5;
            const RowChunks rc = split_row(nvox, want < cap ? want : cap, chunk_min);
            if ((int64_t)rc.nvox != nvox) return 3;
            printf("%" PRId64 " %" PRId64 " %u %u\n", want, cap, rc.chunks, rc.chunk);
        } else if (kind == 'W') {
            unsigned vw, n, same, mis;
            if (scanf("%u %u %u %u", &vw, &n, &same, &mis) != 4 || (vw != 2 && vw != 4)) return 2;
            const WalkSplit w = vw == 2 ? walk_split<2>(n, same != 0, mis) : walk_split<4>(n, same != 0, mis);
            printf("%u %u %u\n", w.head, w.nvec, w.tail);
        } else {
            return 2;
        }
    }
    return 0;
}
