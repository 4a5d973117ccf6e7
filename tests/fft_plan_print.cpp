// Prints the plans of concept_amd/csrc/cg_fft_plan.h for the inputs read from stdin, one request
// per line (tests/test_fft_plan_host.py):
//   chunk N ny pad ncu total
//     -> chunk <layers per chunk> <n> <base> <extra> <begin(0)> ... <begin(n)>
//   choice logn mode N pad ncu split_mode nouter s_es s_sh d_es d_sh
//     -> choice <form> <W> <NT> <lds> <grid> <nkb> <ntiles>
#include <cstdio>
#include <cstring>

#include "cg_fft_plan.h"

int main() {
    static const char *form[] = {"Split", "SplitBlocked", "Persistent", "Plain"};
    char what[16];
    while (scanf("%15s", what) == 1) {
        long long v[11];
        const int want = !strcmp(what, "chunk") ? 5 : !strcmp(what, "choice") ? 11 : -1;
        for (int i = 0; i < want; i++)
            if (scanf("%lld", &v[i]) != 1) return 2;
        if (want == 5) {
            const i64 chunk = zy_chunk_layers(v[0], v[1], v[2], (int)v[3]);
            const ChunkPlan plan(v[4], chunk);
            printf("chunk %lld %lld %lld %lld", (long long)chunk, (long long)plan.n,
                   (long long)plan.base, (long long)plan.extra);
            for (i64 i = 0; i <= plan.n; i++) printf(" %lld", (long long)plan.begin(i));
            printf("\n");
        } else if (want == 11) {
            const StridedChoice s = strided_choice(
                (int)v[0], (int)v[1], v[2], v[3], (int)v[4], (int)v[5], v[6],
                MapShape{v[7], (int)v[8]}, MapShape{v[9], (int)v[10]});
            printf("choice %s %d %d %lld %lld %d %lld\n", form[(int)s.form], s.W, s.NT,
                   (long long)s.lds, (long long)s.grid, s.nkb, (long long)s.ntiles);
        } else {
            return 2;
        }
    }
    return 0;
}
