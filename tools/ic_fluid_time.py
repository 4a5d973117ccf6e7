"""Time one fluid realisation (concept_amd/ic.py: realize of ϱ and J[0..2]) on one GPU, split by
kind of pass: noise (host, wall clock), upload of the noise slab, k-space passes (realize_grid),
inverse transforms and the stores into the fluid grids (fluid_from_mesh), hipEvents around every
pass.

  python tools/ic_fluid_time.py [--gridsize 512] [--runs 2] [--out profiles/ic_fluid_512.json]

A made-up power spectrum: the passes do not depend on the numbers.  The first run warms up
(plans, allocations); the last one is reported.  A record, not a gate."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gridsize', type=int, default=512)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from concept_amd import commons, ic
    from concept_amd.species import Component
    g, L = args.gridsize, 1000.0
    p = commons.load_params({'boxsize': L, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25, 'a_begin': 0.02})
    k = np.geomspace(1e-4, 100, 400)
    amplitudes = 0.01*ic.amplitudes_from_power(k, 2e3*k/(1 + (k/0.1)**2)**1.5, g, L)
    c = Component('matter', 'matter', gridsize=g, boltzmann_order=1)
    record = None
    for _ in range(args.runs):
        timings = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ic.realize(c, p.a_begin, amplitudes, -amplitudes, timings=timings)
        torch.cuda.synchronize()
        record = {'device': torch.cuda.get_device_name(), 'gridsize': g, 'cells': g**3,
                  'variables': ['ϱ', 'J[0]', 'J[1]', 'J[2]'],
                  'wall_ms': (time.perf_counter() - t0)*1e3,
                  'ms': {k_: v for k_, v in timings.items() if not k_.endswith(' passes')},
                  'passes': {k_[:-7]: v for k_, v in timings.items() if k_.endswith(' passes')}}
        record['gpu_ms'] = sum(v for k_, v in record['ms'].items() if k_ != 'noise (host)')
    assert bool(torch.isfinite(c.ϱ).all()) and bool(torch.isfinite(torch.stack(c.J)).all())
    record['delta_rms'] = float((c.ϱ/c.ϱ_bar - 1).std())
    text = json.dumps(record, indent=1, ensure_ascii=False)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(record, ensure_ascii=False))


if __name__ == '__main__':
    main()
