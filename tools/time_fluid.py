"""Time concept_amd.fluid.maccormack with hipEvents: ten calls at grid size 512 (default) on a
smooth fluid, and ten on the same fluid with one void that makes the first step of every call
sweep.  Prints one JSON line (and writes it to --out): the time per call, and the HBM time of
the bytes the passes of a call move at 8 TB/s.

    python tools/time_fluid.py [--gridsize 512] [--calls 10] [--out profiles/fluid_drift_512.json]

Bytes per cell and call, FP64: a step reads five grids and writes four (72 B;
the second step also reads the four it adds to: 104 B); detection reads two grids and writes
fac_time after the first step (24 B), one grid after the second (16 B); the epilogue halves four grids in place (64 B) and clears the four
starred ones (32 B).  A sweep adds the gather (fac_time and the four variables in, four Δ out:
72 B, its neighbour reads served by the caches) and the apply (96 B).  Last, ten source passes of
a w = 0.2 fluid (fluid.internal_sources), 64 B per cell."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8e12   # bytes/s
BYTES_SMOOTH = 72 + 24 + 104 + 16 + 64 + 32   # per cell and call
BYTES_SWEEP = 72 + 96                      # per cell and sweep
BYTES_SOURCES = 8 + 8 + 48                 # per cell and source pass: ϱ in, 𝒫 out, three J in and out
# per cell and Kurganov-Tadmor call of order 2: either step reads four grids and writes four and
# 𝒫 (72 B); the second also reads the four it adds to (32 B)
BYTES_KT = 72 + 72 + 32


def fields(gs, void, device):
    q = (torch.arange(gs, dtype=torch.float64, device=device) + 0.5)*(2*np.pi/gs)
    x, y, z = q[:, None, None], q[None, :, None], q[None, None, :]
    ϱ = 1 + 0.3*torch.sin(x)*torch.cos(y + 0.4) + 0.1*torch.sin(2*z + x)
    u = [0.35*torch.sin(y + 0.3) + 0.2*torch.cos(z) + 0*x, -0.3*torch.cos(x + z) + 0.1 + 0*y,
         0.25*torch.sin(x - y) - 0.15 + 0*z]
    J = [ϱ*u_d for u_d in u]
    if void:
        h = gs//2
        ϱ[h:h + 2, h:h + 2, h:h + 2] = 0.3
        for d in range(3):
            J[d][h:h + 2, h:h + 2, h:h + 2] = 0
    return ϱ.contiguous(), [j.contiguous() for j in J]


def time_kt(args):
    """--kt: ten kurganov_tadmor calls of order 2 (w = 0.2, 'mc') beside the MacCormack line of
    profiles/fluid_drift_512.json and the HBM time of the bytes of a call"""
    from concept_amd import commons, fluid
    from concept_amd.species import Component
    gs = args.gridsize
    commons.load_params({'boxsize': float(gs), 'select_eos_w': {'all': 0.2},
                         'select_approximations': {'P=wρ': True}, 'enable_Hubble': False,
                         'fluid_scheme_select': 'Kurganov-Tadmor',
                         'fluid_options': {'kurganovtadmor': {'flux_limiter_select': 'mc'}}})
    device = torch.device('cuda', torch.cuda.current_device())
    c = Component('fluid', 'matter', gridsize=gs, boltzmann_order=1)
    ϱ, J = fields(gs, False, device)
    c.ϱ.copy_(ϱ)
    for d in range(3):
        c.J[d].copy_(J[d])
    del ϱ, J
    # a Courant number of about 0.07 on a grid spacing of 1 (the sound speed is c sqrt(0.2))
    ᔑdt = {'1': 5e-4, ('a**(3*w_eff-2)', c.name): 5e-4, ('a**(-3*w_eff)', c.name): 5e-4}
    fluid.kurganov_tadmor(c, ᔑdt, 1.0, rk_order=2)   # warm-up: buffers, first launches
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.calls):
        fluid.kurganov_tadmor(c, ᔑdt, 1.0, rk_order=2)
    end.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(end)/args.calls
    hbm_ms = gs**3*BYTES_KT/HBM_PEAK*1e3
    result = {'gridsize': gs, 'calls': args.calls, 'device': torch.cuda.get_device_name(device),
              'hbm_peak_TBps': HBM_PEAK/1e12,
              'kurganov_tadmor': {
                  'rk_order': 2, 'limiter': 'mc', 'w': 0.2, 'ms_per_call': round(ms, 4),
                  'bytes_per_call': int(gs**3*BYTES_KT), 'hbm_ms_at_8TBps': round(hbm_ms, 4),
                  'fraction_of_hbm_rate': round(hbm_ms/ms, 4),
                  'min_rho': float(c.ϱ.min().item())}}
    recorded = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            'profiles', 'fluid_drift_512.json')
    if gs == 512 and os.path.exists(recorded):
        with open(recorded) as f:
            result['maccormack_smooth_recorded'] = json.load(f)['smooth']
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gridsize', type=int, default=512)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kt', action='store_true',
                    help='time the Kurganov-Tadmor scheme instead (profiles/fluid_kt_512.json)')
    args = ap.parse_args()
    if args.kt:
        line = json.dumps(time_kt(args))
        print(line)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(line + '\n')
        return
    from concept_amd import commons, fluid
    from concept_amd.species import Component
    gs = args.gridsize
    commons.load_params({'boxsize': float(gs)})
    device = torch.device('cuda', torch.cuda.current_device())
    result = {'gridsize': gs, 'calls': args.calls, 'device': torch.cuda.get_device_name(device),
              'hbm_peak_TBps': HBM_PEAK/1e12}
    for void in (False, True):
        c = Component('fluid', 'matter', gridsize=gs, boltzmann_order=1)
        ϱ, J = fields(gs, void, device)
        c.ϱ.copy_(ϱ)
        for d in range(3):
            c.J[d].copy_(J[d])
        del ϱ, J
        # a Courant number of about 0.05 on a grid spacing of 1
        ᔑdt = {'1': 0.1, ('a**(3*w_eff-2)', c.name): 0.1}
        fluid.reset_steps()
        fluid.maccormack(c, ᔑdt)   # warm-up: buffers, first launches
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sweeps = 0
        start.record()
        for _ in range(args.calls):
            fluid.maccormack(c, ᔑdt)
            sweeps += sum(c.maccormack_sweeps)
        end.record()
        torch.cuda.synchronize()
        ms = start.elapsed_time(end)/args.calls
        moved = gs**3*(BYTES_SMOOTH + BYTES_SWEEP*sweeps/args.calls)
        hbm_ms = moved/HBM_PEAK*1e3
        result['void' if void else 'smooth'] = {
            'ms_per_call': round(ms, 4), 'sweeps_per_call': sweeps/args.calls,
            'bytes_per_call': int(moved), 'hbm_ms_at_8TBps': round(hbm_ms, 4),
            'fraction_of_hbm_rate': round(hbm_ms/ms, 4),
            'min_rho': float(c.ϱ.min().item())}
        del c
        torch.cuda.empty_cache()
    # the source pass of a w = 0.2 fluid (fluid.internal_sources: 𝒫 = ϱ c²w and the pressure term
    # of the Euler equation in one pass): reads ϱ, writes 𝒫, reads and writes three J grids
    commons.load_params({'boxsize': float(gs), 'select_eos_w': {'all': 0.2},
                         'select_approximations': {'P=wρ': True}})
    c = Component('fluid', 'matter', gridsize=gs, boltzmann_order=1)
    ϱ, J = fields(gs, False, device)
    c.ϱ.copy_(ϱ)
    for d in range(3):
        c.J[d].copy_(J[d])
    del ϱ, J
    ᔑdt = {'1': 1e-6, ('a**(-3*w_eff)', c.name): 1e-6}
    fluid.internal_sources(c, ᔑdt)
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.calls):
        fluid.internal_sources(c, ᔑdt)
    end.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(end)/args.calls
    hbm_ms = gs**3*BYTES_SOURCES/HBM_PEAK*1e3
    result['pressure_sources'] = {
        'ms_per_call': round(ms, 4), 'bytes_per_call': int(gs**3*BYTES_SOURCES),
        'hbm_ms_at_8TBps': round(hbm_ms, 4), 'fraction_of_hbm_rate': round(hbm_ms/ms, 4)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
