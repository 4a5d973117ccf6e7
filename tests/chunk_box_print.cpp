// Prints the integer arithmetic of concept_amd/csrc/cg_chunk_box.h for the requests read from
// stdin, one per line (tests/test_chunk_box_host.py).  W, H: the stencil's width and how far below
// the particle's cell it starts; r, lo, hi: the reference cell and the extremes of the particles'
// cells relative to it, three numbers each.
//   rel N                       -> rel <chunk_rel(cell, ref, N) for cell < N for ref < N>
//   box W H N r lo hi           -> box <fits> <e0> <e1> <e2> <ncells> <the cell of every entry>
//   entries W H N r lo hi m <m cells>
//                               -> entries <entry_of(cell) for each cell>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "cg_chunk_box.h"

template <int W, int H>
static void answer(bool entries, int N, const int (&r)[3], const int (&lo)[3], const int (&hi)[3]) {
    ChunkBox<W, H> B;
    B.set(r, lo, hi, N);
    if (!entries) {
        printf("box %d %d %d %d %d", (int)B.fits, B.e[0], B.e[1], B.e[2], B.ncells());
        for (int i = 0; i < B.ncells(); i++) {
            int cell[3];
            B.cell_of(i, N, cell);
            printf(" %d %d %d", cell[0], cell[1], cell[2]);
        }
    } else {
        int m = 0;
        if (scanf("%d", &m) != 1) return;
        printf("entries");
        for (int i = 0; i < m; i++) {
            int cell[3];
            if (scanf("%d %d %d", &cell[0], &cell[1], &cell[2]) != 3) return;
            printf(" %d", B.entry_of(cell, N));
        }
    }
    printf("\n");
}

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "rel")) {
            int N;
            if (scanf("%d", &N) != 1) return 2;
            printf("rel");
            for (int ref = 0; ref < N; ref++)
                for (int cell = 0; cell < N; cell++) printf(" %d", chunk_rel(cell, ref, N));
            printf("\n");
            continue;
        }
        const bool entries = !strcmp(what, "entries");
        if (!entries && strcmp(what, "box")) return 2;
        int W, H, N, r[3], lo[3], hi[3];
        if (scanf("%d %d %d", &W, &H, &N) != 3) return 2;
        for (int *v : {r, lo, hi})
            if (scanf("%d %d %d", &v[0], &v[1], &v[2]) != 3) return 2;
        switch (10 * W + H) {
            case 10: answer<1, 0>(entries, N, r, lo, hi); break;
            case 20: answer<2, 0>(entries, N, r, lo, hi); break;
            case 30: answer<3, 0>(entries, N, r, lo, hi); break;
            case 40: answer<4, 0>(entries, N, r, lo, hi); break;
            case 41: answer<4, 1>(entries, N, r, lo, hi); break;
            case 62: answer<6, 2>(entries, N, r, lo, hi); break;
            default: return 2;
        }
    }
    return 0;
}
