"""Time the bispectrum core: one run of equilateral bins on one GPU, hipEvents around the
three phases of every grid (shell fill, backward FFT) and of every bin (sums).

  python tools/time_bispec.py [--gridsize 512] [--bins 20] [--out profiles/bispec_512.json]

The bins are equilateral (three equal shells, so one grid per bin) with the reference's
default thickness max(3, log(10)/20 k) in grid units, centred on k spread evenly in log over
[3, nyquist - 3], antialiasing on, data fields of a random slab.  Every time is set against
the HBM time of the bytes the phase has to move at 8 TB/s.  A record, not a gate."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gridsize', type=int, default=512)
    ap.add_argument('--bins', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from concept_amd import analysis, commons
    commons.load_params({'boxsize': 100.0})
    N, nyq = args.gridsize, args.gridsize//2
    slab = analysis._mesh(N, 'bispec')
    grid = analysis._mesh(N, 'bispec 0')
    gen = torch.Generator(device=slab.device).manual_seed(1)
    field = 1 + 0.5*torch.randn(N**3, dtype=torch.float64, device=slab.device, generator=gen)
    slab.fluid_add(field*float(N)**-3, 1.0, '=')
    slab.fft_forward()
    del field
    ks = np.exp(np.linspace(math.log(3.0), math.log(nyq - 3.0), args.bins))
    shells = [(k - 0.5*max(3, math.log(10)/20*k), k + 0.5*max(3, math.log(10)/20*k)) for k in ks]
    out = torch.empty(4, dtype=torch.float64, device=slab.device)

    def one(shell, events):
        events[0].record()
        grid.bispec_shell(shell, slab, True)
        events[1].record()
        grid.poisson_backward()
        events[2].record()
        grid.bispec_sums((), 1, out=out)
        events[3].record()
    one(shells[0], [torch.cuda.Event(enable_timing=True) for _ in range(4)])   # warm-up
    rows = []
    for shell in shells:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        one(shell, ev)
        ev[3].synchronize()
        rows.append([ev[i].elapsed_time(ev[i + 1]) for i in range(3)] + out.cpu().tolist()[:2])
    t = np.array(rows)
    cp = slab.pad//2
    view_bytes = N*N*cp*16
    real_bytes = N**3*8
    # shell fill: writes the view, reads the source inside the shell (at most the view);
    # backward FFT: three passes that each read and write the mesh; sums: one read of one grid
    floor_ms = {'shell_fill': 1e3*view_bytes/HBM_BYTES_PER_S,
                'backward_fft': 1e3*6*view_bytes/HBM_BYTES_PER_S,
                'sums': 1e3*real_bytes/HBM_BYTES_PER_S}
    record = {
        'device': torch.cuda.get_device_name(slab.device), 'gridsize': N, 'bins': args.bins,
        'antialiasing': True, 'unique_grids_per_bin': 1,
        'shells': [[float(a), float(b)] for a, b in shells],
        'ms_per_bin': {'shell_fill': t[:, 0].tolist(), 'backward_fft': t[:, 1].tolist(),
                       'sums': t[:, 2].tolist()},
        'ms_median': {'shell_fill': float(np.median(t[:, 0])),
                      'backward_fft': float(np.median(t[:, 1])),
                      'sums': float(np.median(t[:, 2]))},
        'ms_max': {'shell_fill': float(t[:, 0].max()), 'backward_fft': float(t[:, 1].max()),
                   'sums': float(t[:, 2].max())},
        'hbm_floor_ms_at_8TBps': floor_ms,
        'value': t[:, 3].tolist(), 'power': t[:, 4].tolist(),
    }
    text = json.dumps(record, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps({k: record[k] for k in ('gridsize', 'bins', 'ms_median', 'ms_max',
                                             'hbm_floor_ms_at_8TBps')}))


if __name__ == '__main__':
    main()
