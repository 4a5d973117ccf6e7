#!/usr/bin/env python3
"""Write tests/golden/pp_ewald_mp.npz: the Ewald correction table (ewald.py:62-118, 226-271) in
40-digit mpmath (tests/pp_refs.py ewald_summation_mp), at every point of tables of size 2, 3,
4 and 5 and at a fixed list of points of the default table of size 64.

Per size g: points_g (n, 3) grid indices, hi_g + lo_g (n, 3) the mp value split into two
float64, S_g (n, 3) the sum of the absolute values of the terms (|sin| taken as 1).
k_oracle: the largest |oracle - mp| / (2^-53 S) over all of them, oracle.pp.ewald_tabulate on
the CPU being the oracle — what a correct float64 evaluation with the host's erfc/exp/sin
reaches.  The GPU test allows K = max(4 k_oracle, 32).

    python tests/golden/make_golden_pp_ewald.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

POINTS_64 = [(0, 0, 1), (1, 0, 0), (1, 1, 1), (63, 63, 63), (63, 0, 0), (0, 63, 31),
             (32, 32, 32), (0, 0, 63), (0, 1, 1), (1, 1, 0), (2, 0, 0), (0, 0, 2), (1, 2, 3),
             (5, 5, 5), (0, 32, 0), (31, 0, 63), (63, 63, 0), (63, 62, 61), (17, 42, 5),
             (62, 1, 33)]


def main():
    import mpmath as mp
    import pp_refs
    from oracle import pp
    out = {}
    k_oracle = 0.0
    for g in (2, 3, 4, 5, 64):
        pts = (POINTS_64 if g == 64 else
               [(i, j, k) for i in range(g) for j in range(g) for k in range(g)])
        table = pp.ewald_tabulate(g)
        hi = np.zeros((len(pts), 3))
        lo = np.zeros_like(hi)
        S = np.zeros_like(hi)
        for n, p in enumerate(pts):
            f, s = pp_refs.ewald_summation_mp(*(pp_refs.table_coordinate(i, g) for i in p))
            with mp.workdps(40):
                for d in range(3):
                    hi[n, d] = float(f[d])
                    lo[n, d] = float(f[d] - mp.mpf(hi[n, d]))
                    S[n, d] = float(s[d])
                    if s[d] > 0:
                        ratio = abs(mp.mpf(float(table[p][d])) - f[d])/(mp.mpf(2)**-53*s[d])
                        k_oracle = max(k_oracle, float(ratio))
                    else:
                        assert table[p][d] == 0
        out[f'points_{g}'] = np.array(pts, dtype=np.int64)
        out[f'hi_{g}'], out[f'lo_{g}'], out[f'S_{g}'] = hi, lo, S
        print(f'size {g}: {len(pts)} points, k_oracle so far {k_oracle:.3f}', flush=True)
    out['k_oracle'] = np.float64(k_oracle)
    np.savez_compressed(os.path.join(HERE, 'pp_ewald_mp.npz'), **out)
    print('wrote pp_ewald_mp.npz, k_oracle =', k_oracle)


if __name__ == '__main__':
    main()
