"""Time the shear term of closure 'class' (concept_amd/fluid.py: shear_sources) on one GPU, split by
kind of pass: the structure (ϱ into a mesh and its forward transform), the three k-space passes
(cg_shear_divergence), the three inverse transforms and the three accumulating stores, hipEvents
around every pass; beside it the six-grid route of the reference as far as it is built here
(ic.realize_shear six times from one structure: six k-space passes, six inverse transforms, six
stores, without the differences that would follow).

  python tools/shear_time.py [--gridsizes 256 512] [--runs 3] [--out profiles/fluid_shear.json]

A made-up density and table: the passes do not depend on the numbers.  The first runs warm up
(plans, allocations); the last one is reported.  A record, not a gate."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(g, runs):
    from concept_amd import commons, fluid, ic, mesh
    from concept_amd.species import Component
    L = 1000.0
    commons.load_params({'boxsize': L, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25,
                         'select_eos_w': {'nu': 1/3},
                         'select_approximations': {'all': {'P=wρ': True}},
                         'select_boltzmann_closure': {'nu': 'class'},
                         'realization_options': {'structure': {'nu': 'nonlinear'}}})
    c = Component('nu', 'neutrino', gridsize=g, boltzmann_order=1)
    torch.manual_seed(g)
    c.ϱ.copy_(2.5*(1 + 0.1*(2*torch.rand_like(c.ϱ) - 1)))
    k = np.geomspace(1e-4, 100, 50)
    table = ic.amplitudes_from_transfer_ratio(k, -0.3/(1 + k), g, L, c.ϱ_bar)
    ᔑdt = {'1': 0.01, ('a**(-3*w_eff)', c.name): 0.01}
    for _ in range(runs):
        timings = {}
        fluid.shear_sources(c, ᔑdt, table, 0.5, timings=timings)
    assert bool(torch.isfinite(torch.stack(c.J)).all())
    record = {'gridsize': g, 'cells': g**3,
              'ms': {k_: v for k_, v in timings.items() if not k_.endswith(' passes')},
              'passes': {k_[:-7]: v for k_, v in timings.items() if k_.endswith(' passes')}}
    record['total_ms'] = sum(record['ms'].values())
    out = torch.empty_like(c.ϱ)
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    for _ in range(runs):
        e0.record()
        structure = ic.fluid_structure(c)
        for m in range(3):
            for n in range(m, 3):
                ic.realize_shear(c, 0.5, table, (m, n), structure=structure, out=out)
        e1.record()
        torch.cuda.synchronize()
    record['six_grids_ms'] = e0.elapsed_time(e1)
    del c, out
    mesh.free_meshes()
    torch.cuda.empty_cache()
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gridsizes', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    record = {'device': torch.cuda.get_device_name(),
              'runs': [measure(g, args.runs) for g in args.gridsizes]}
    for run in record['runs']:
        print(f"{run['gridsize']}³: " + ', '.join(f'{k} {v:.3f} ms' for k, v in run['ms'].items())
              + f"; total {run['total_ms']:.3f} ms; six ς grids {run['six_grids_ms']:.3f} ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(record, indent=1, ensure_ascii=False) + '\n')
    print(json.dumps(record, ensure_ascii=False))


if __name__ == '__main__':
    main()
