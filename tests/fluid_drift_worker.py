"""Worker of tests/test_gpu_fluid_drift.py: one rank of a P-rank x-slab run of the fluid solver.
The ranks share cuda:0 and talk over gloo (test only; production is one GPU per rank over RCCL).
Every rank holds its own layers of the fluid, exchanges the neighbour layers the step and the
sweep read, and the gathered grids must agree with the reference's goldens — and so with one
domain — at the same bar."""
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
    import test_gpu_fluid_drift as t
    for name in sys.argv[1:]:
        worst = t.run_drift_golden(name, tag=f'rank {rank}/{world} ')
        print(f'rank {rank}: {name} ok ({worst:.3e})', flush=True)
    dist.barrier()
    print(f'RANK{rank}-OK', flush=True)


if __name__ == '__main__':
    main()
