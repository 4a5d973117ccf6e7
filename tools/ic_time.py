"""Time one particle realisation (concept_amd/ic.py) on one GPU, split by kind of pass:
noise (host, wall clock) and upload of the noise slab, or with --noise-on device the noise drawn
on the GPU (stream table on the host and kernel), k-space passes (lpt_potential, lpt_diff),
transforms, grid products and particle passes (lattice, displacement, wrap), hipEvents around
every pass.

  python tools/ic_time.py [--gridsize 512] [--lpt 2] [--dealias] [--runs 2] [--fused]
                          [--noise-on host|device] [--out profiles/ic_512.json]

--lpt 3 and --dealias go through realize_particles(extended=True).  --fused also times, on the
realisation's own meshes in this process, each of the three passes between the realisation size N
and the dealiasing size M against the unfused passes it replaces: lpt_diff + zero_fourier +
copy_modes_from for lpt_diff_enlarge, copy_modes_from into a nullified slab + an accumulation
for lpt_shrink_accumulate, nothing shorter than itself for lpt_dealias_cube (listed with the
whole-slab zeroing for scale); median of 5 after a warm-up, hipEvents.

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


def fused_vs_unfused(grids, p, device):
    from concept_amd.mesh import get_mesh
    n, m = grids['gridsize'], grids['gridsize_dealias']
    if m == n:
        raise SystemExit('--fused needs --dealias')

    def mesh(role, size):
        return get_mesh(size, p.boxsize, p.nghosts, p.cell_centered, role=role, device=device)
    Φ, tmp, out = grids['Φ1'], mesh('lpt tmp0', n), mesh('lpt tmp1', n)
    big = mesh('lpt tmp0 dealias', m)

    def median_ms(f):
        f()
        times = []
        for _ in range(5):
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return sorted(times)[2]

    def enlarge_unfused():
        tmp.lpt_diff(Φ, 0, 1)
        big.copy_modes_from(tmp)  # zero_fourier, then the copy with the phase

    def shrink_unfused():
        tmp.copy_modes_from(big)  # the same into a slab of size N
        out.fourier_operate(source=tmp, operation='+=')

    slab_bytes = {'N': 8*n*n*(n + 2), 'M': 8*m*m*(m + 2)}
    ms = {'diff_enlarge fused': median_ms(lambda: big.lpt_diff_enlarge(Φ, 0, 1)),
          'diff_enlarge unfused': median_ms(enlarge_unfused),
          'shrink_accumulate fused': median_ms(lambda: out.lpt_shrink_accumulate(big, '+=', 0.5)),
          'shrink_accumulate unfused': median_ms(shrink_unfused),
          'dealias_cube': median_ms(lambda: big.lpt_dealias_cube(n)),
          'zero_fourier (M)': median_ms(big.zero_fourier)}
    # what the expectation prices: one write of the M slab (enlarge), one read of the cube's
    # part of it plus read and write of the N slab (shrink), the write of M less the cube (cube)
    ms['slab bytes'] = slab_bytes
    ms['TB/s'] = {
        'diff_enlarge fused': (slab_bytes['N'] + slab_bytes['M'])/ms['diff_enlarge fused']/1e9,
        'shrink_accumulate fused': 3*slab_bytes['N']/ms['shrink_accumulate fused']/1e9,
        'dealias_cube': (slab_bytes['M'] - slab_bytes['N'])/ms['dealias_cube']/1e9}
    return ms


def noise_kernel(g, p, device):
    """the noise kernel alone (tables already on the device): median of 5 after a warm-up, and its
    rate in raw words of PCG64DXSM, one per phase and what the ziggurat took per amplitude"""
    from concept_amd import ic, lib
    from concept_amd.mesh import get_mesh
    mesh = get_mesh(g, p.boxsize, p.nghosts, p.cell_centered, role='lpt tmp0', device=device)
    trip = int(lib.raw().cg_noise_trip())
    streams = torch.from_numpy(ic.noise_stream_table(g, False, p).view(np.int64)).to(device)
    order = torch.from_numpy(ic.noise_order_table(g)).to(device)
    jump = torch.from_numpy(ic.pcg64dxsm_jump_table(trip).view(np.int64)).to(device)
    times = []
    for _ in range(6):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        mesh.noise_generate(streams, order, jump, p.primordial_amplitude_fixed,
                            p.primordial_phase_shift)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = sorted(times[1:])[2]
    draws = (g - 1)*((g - 1)*g//2)
    # a trip of `trip` words makes about trip/1.02 amplitudes: the words the kernel hashes
    trips = -(-int(draws/(g - 1)*1.0235)//trip)
    words = (g - 1)*trips*trip + draws
    return {'ms': ms, 'draws per stream kind': draws, 'raw words (estimate)': words,
            'raw words per second': words/(ms*1e-3), 'trip': trip}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gridsize', type=int, default=512)
    ap.add_argument('--lpt', type=int, default=2)
    ap.add_argument('--dealias', action='store_true')
    ap.add_argument('--fused', action='store_true')
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--noise-on', choices=('host', 'device'), default='host')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from concept_amd import commons, ic
    from concept_amd.species import Component
    g, L = args.gridsize, 1000.0
    p = commons.load_params({
        'boxsize': L, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25, 'a_begin': 0.02,
        'potential_options': {'gridsize': {'gravity': {'pm': g}}},
        'select_forces': {'all': {'gravity': 'pm'}},
        'realization_options': {'lpt': args.lpt, 'backscale': True, 'dealias': args.dealias}})
    extended = args.lpt > 2 or args.dealias
    k = np.geomspace(1e-4, 100, 400)
    amplitudes = ic.amplitudes_from_power(k, 2e3*k/(1 + (k/0.1)**2)**1.5, g, L)
    growth = {'D1': 0.02, 'f1': 1.0, 'D2': -3/7*0.02**2, 'f2': 2.0}
    if args.lpt > 2:
        growth.update({'D3a': -1/3*0.02**3, 'f3a': 3.0, 'D3b': 10/21*0.02**3, 'f3b': 3.0,
                       'D3c': -1/7*0.02**3, 'f3c': 3.0})
    c = Component('matter', 'matter', N=g**3, mass=-1)
    c.keep_order = False
    record = None
    for _ in range(args.runs):
        ic.reset_tally()
        timings = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grids = ic.realize_particles(c, p.a_begin, amplitudes, growth_factors=growth,
                                     timings=timings, **({'extended': True} if extended else {}),
                                     **({'noise_on': 'device'} if args.noise_on == 'device'
                                        else {}))
        torch.cuda.synchronize()
        record = {'device': torch.cuda.get_device_name(), 'gridsize': g, 'particles': g**3,
                  'lpt': args.lpt, 'backscale': True, 'dealias': args.dealias,
                  'noise_on': args.noise_on,
                  'gridsize_dealias': grids.get('gridsize_dealias', g),
                  'wall_ms': (time.perf_counter() - t0)*1e3,
                  'ms': {k_: v for k_, v in timings.items() if not k_.endswith(' passes')},
                  'passes': {k_[:-7]: v for k_, v in timings.items() if k_.endswith(' passes')}}
        record['gpu_ms'] = sum(v for k_, v in record['ms'].items() if k_ != 'noise (host)')
    assert bool(((c.pos >= 0) & (c.pos < L)).all())
    if args.noise_on == 'device':
        record['noise_kernel'] = noise_kernel(g, p, c.device)
    if args.fused:
        record['fused_vs_unfused_ms'] = fused_vs_unfused(grids, p, c.device)
    text = json.dumps(record, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(record))


if __name__ == '__main__':
    main()
