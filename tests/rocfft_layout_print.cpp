// Prints the layouts of concept_amd/csrc/cg_rocfft_layout.h for the inputs read from stdin, one
// request per line (tests/test_rocfft_layout_host.py):
//   <plan> inverse N ny pad nprocs nlayers      plan: 3d, 2d, z, y or x
//     -> <plan> <kind> <dims> <batch> <in_dist> <out_dist> <length, in_stride, out_stride> per
//        dimension, fastest first
#include <cstdio>
#include <cstring>

#include "cg_rocfft_layout.h"

int main() {
    static const char *kind[] = {"RealForward", "RealInverse", "ComplexForward", "ComplexInverse"};
    char what[16];
    while (scanf("%15s", what) == 1) {
        unsigned long long v[6];
        for (auto &x : v)
            if (scanf("%llu", &x) != 1) return 2;
        const bool inverse = v[0] != 0;
        const size_t N = v[1], ny = v[2], pad = v[3], nprocs = v[4], nlayers = v[5];
        RocfftLayout l;
        if (!strcmp(what, "3d")) l = fft_layout_3d(inverse, N, ny, pad);
        else if (!strcmp(what, "2d")) l = fft_layout_2d(inverse, N, ny, pad, nlayers);
        else if (!strcmp(what, "z")) l = fft_layout_z_rows(inverse, N, pad);
        else if (!strcmp(what, "y")) l = fft_layout_y_columns(inverse, N, pad);
        else if (!strcmp(what, "x")) l = fft_layout_x(inverse, N, pad, nprocs);
        else return 2;
        printf("%s %s %zu %zu %zu %zu", what, kind[(int)l.kind], l.dims, l.batch, l.in_dist,
               l.out_dist);
        for (size_t d = 0; d < l.dims; d++)
            printf(" %zu %zu %zu", l.lengths[d], l.in_stride[d], l.out_stride[d]);
        printf("\n");
    }
    return 0;
}
