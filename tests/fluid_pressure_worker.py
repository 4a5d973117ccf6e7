"""Worker of tests/test_gpu_fluid_pressure.py: one rank of a P-rank x-slab run of the pressure
term.  The ranks share cuda:0 and talk over gloo (test only; production is one GPU per rank over
RCCL).  Every rank holds its own layers of the fluid and exchanges the one neighbour layer of ϱ
that the stencil reads; the gathered grids must meet the golden at the same bar and equal the
one-domain result bit for bit.
  golden ONE.npz   fluid_pressure_sources_g8; ONE.npz holds J and P of the one-domain run
  seams            the random fields on grid size 40 against the NumPy restatement"""
import os
import sys

import numpy as np
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
    import test_gpu_fluid_pressure as t
    tag = f'rank {rank}/{world} '
    if sys.argv[1] == 'golden':
        worst, J, 𝒫 = t.run_sources_golden(tag=tag)
        one = np.load(sys.argv[2])
        same = np.array_equal(J, one['J']) and np.array_equal(𝒫, one['P'])
        print(f'{tag}golden ok ({worst:.3e}), bit-identical to one domain: {same}', flush=True)
        assert same
    else:
        worst = t.run_seams(tag=tag)
        print(f'{tag}seams ok ({worst:.3e})', flush=True)
    dist.barrier()
    print(f'RANK{rank}-OK', flush=True)


if __name__ == '__main__':
    main()
