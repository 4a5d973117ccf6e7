// Host program around concept_amd/csrc/cg_bispec.h (tests/test_bispec_host.py builds it with
// the host C++ compiler alone).
//   bispec_overlap_main overlap FILE   per line "ki kj kk k_inner k_outer": the overlap
//   bispec_overlap_main rows N k_inner k_outer   per array row (a, b): visited kk_bgn kk_end
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cg_bispec.h"

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "overlap")) {
        FILE *f = fopen(argv[2], "r");
        if (!f) return 2;
        long long ki, kj, kk;
        double k_inner, k_outer;
        while (fscanf(f, "%lld %lld %lld %lf %lf", &ki, &kj, &kk, &k_inner, &k_outer) == 5)
            printf("%.17g\n", bispec_overlap_cellshell(ki, kj, kk, k_inner, k_outer));
        fclose(f);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "rows")) {
        const int64_t N = atoll(argv[2]), nyq = N / 2;
        const BispecShellBounds b = bispec_shell_bounds(N, atof(argv[3]), atof(argv[4]));
        for (int64_t a = 0; a < N; a++)
            for (int64_t bb = 0; bb < N; bb++) {
                int64_t bgn = 0, end = -1;
                const bool v = bispec_shell_row(b, a - (a >= nyq ? N : 0),
                                                bb - (bb >= nyq ? N : 0), &bgn, &end);
                printf("%d %lld %lld\n", (int)v, (long long)bgn, (long long)end);
            }
        return 0;
    }
    fprintf(stderr, "usage: %s overlap FILE | rows N k_inner k_outer\n", argv[0]);
    return 1;
}
