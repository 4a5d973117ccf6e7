"""Worker of tests/test_gpu_bispec.py: one rank of a P-rank x-slab bispectrum measurement.  The
ranks share cuda:0 and talk over gloo (test only; production is one GPU per rank over RCCL).
Every rank fills and sums its own part; the sums are combined in rank order, so every rank
holds the result, which rank 0 prints as one JSON line."""
import json
import os
import sys

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def main():
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from concept_amd import comm
    comm.init()
    import test_gpu_bispec as t
    out = {}
    for antialiasing in (True, False):
        res = t.measure(antialiasing)
        out['aa' if antialiasing else 'noaa'] = {k: getattr(res, k).tolist()
                                                 for k in res._fields}
    dist.barrier()
    if rank == 0:
        print('RESULT ' + json.dumps(out), flush=True)
    print(f'RANK{rank}-OK', flush=True)


if __name__ == '__main__':
    main()
