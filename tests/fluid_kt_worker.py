"""Worker of tests/test_gpu_fluid_kt.py: one rank of a P-rank x-slab run of the Kurganov-Tadmor
step.  The ranks share cuda:0 and talk over gloo (test only; production is one GPU per rank over
RCCL).  Every rank holds its own layers of the fluid and exchanges the two neighbour layers of ϱ
and J that the stencil reads; the gathered grids must meet the bar and equal the one-domain result
bit for bit.
  golden NAME ONE.npz   the drift calls of golden NAME; ONE.npz holds rho, J and P of the
                        one-domain run
  seams GS LIMITER      the random fields on grid size GS against the NumPy restatement"""
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
    import test_gpu_fluid_kt as t
    tag = f'rank {rank}/{world} '
    if sys.argv[1] == 'golden':
        worst, ϱ, J, 𝒫 = t.run_golden(sys.argv[2], tag=tag)
        one = np.load(sys.argv[3])
        same = (np.array_equal(ϱ, one['rho']) and np.array_equal(J, one['J'])
                and np.array_equal(𝒫, one['P']))
        print(f'{tag}golden ok ({worst:.3e}), bit-identical to one domain: {same}', flush=True)
        assert same
    else:
        worst = t.run_seams(int(sys.argv[2]), sys.argv[3], tag=tag)[0]
        print(f'{tag}seams ok ({worst:.3e})', flush=True)
    dist.barrier()
    print(f'RANK{rank}-OK', flush=True)


if __name__ == '__main__':
    main()
