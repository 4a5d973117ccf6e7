"""Time one particle realisation (concept_amd/ic.py) on one GPU, split by kind of pass:
noise (host, wall clock), upload of the noise slab, k-space passes (lpt_potential, lpt_diff),
transforms, grid products and particle passes (lattice, displacement, wrap), hipEvents around
every pass.

  python tools/ic_time.py [--gridsize 512] [--lpt 2] [--runs 2] [--out profiles/ic_512.json]

A made-up power spectrum, back-scaling on, fixed growth factors: the passes do not depend on
the numbers.  The first run warms up (plans, allocations); the last one is reported.  A record,
not a gate."""
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
    ap.add_argument('--lpt', type=int, default=2)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from concept_amd import commons, ic
    from concept_amd.species import Component
    g, L = args.gridsize, 1000.0
    p = commons.load_params({
        'boxsize': L, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25, 'a_begin': 0.02,
        'potential_options': {'gridsize': {'gravity': {'pm': g}}},
        'select_forces': {'all': {'gravity': 'pm'}},
        'realization_options': {'lpt': args.lpt, 'backscale': True}})
    k = np.geomspace(1e-4, 100, 400)
    amplitudes = ic.amplitudes_from_power(k, 2e3*k/(1 + (k/0.1)**2)**1.5, g, L)
    growth = {'D1': 0.02, 'f1': 1.0, 'D2': -3/7*0.02**2, 'f2': 2.0}
    c = Component('matter', 'matter', N=g**3, mass=-1)
    c.keep_order = False
    record = None
    for _ in range(args.runs):
        ic.reset_tally()
        timings = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ic.realize_particles(c, p.a_begin, amplitudes, growth_factors=growth, timings=timings)
        torch.cuda.synchronize()
        record = {'device': torch.cuda.get_device_name(), 'gridsize': g, 'particles': g**3,
                  'lpt': args.lpt, 'backscale': True,
                  'wall_ms': (time.perf_counter() - t0)*1e3,
                  'ms': {k_: v for k_, v in timings.items() if not k_.endswith(' passes')},
                  'passes': {k_[:-7]: v for k_, v in timings.items() if k_.endswith(' passes')}}
        record['gpu_ms'] = sum(v for k_, v in record['ms'].items() if k_ != 'noise (host)')
    assert bool(((c.pos >= 0) & (c.pos < L)).all())
    text = json.dumps(record, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(record))


if __name__ == '__main__':
    main()
