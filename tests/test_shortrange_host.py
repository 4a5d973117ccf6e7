"""Host logic of the short-range sweep's dispatch (no GPU): the rows the sweep without a cell
list takes (commons.sparse_rows) do not depend on the rung populations, which may lag behind
the rung array — every set row comes back, no slot handed on names a row outside the array,
and more rows than the sweep takes are visible in its last slot."""
import numpy as np
import pytest

SPARSE_MAX = 8   # PotentialMesh.SHORTRANGE_SPARSE_MAX


@pytest.mark.parametrize('n_set', range(13))
def test_sparse_rows_whatever_the_populations_claim(n_set):
    import torch
    from concept_amd import commons
    n = 40
    rng = np.random.default_rng(n_set)
    truth = np.sort(rng.choice(n, n_set, replace=False))
    mask = torch.zeros(n, dtype=torch.bool)
    mask[torch.as_tensor(truth, dtype=torch.int64)] = True
    # (the populations no longer enter: the rows are the same whatever they claim — what
    # torch.nonzero_static(mask, size=claimed) gave before: padded with -1 when they overstate,
    # cut short when they understate)
    rows = commons.sparse_rows(mask, SPARSE_MAX)
    assert rows.dtype == torch.int64 and rows.shape == (SPARSE_MAX + 1,)
    got = rows.numpy()
    valid = got[got >= 0]
    assert np.all((got >= 0) | (got == -1))
    assert np.all(valid < n)
    # the set rows first, in order, the empty slots after them
    assert np.array_equal(got[:valid.size], valid)
    assert np.array_equal(valid, truth[:SPARSE_MAX + 1])
    # the sweep takes the first SPARSE_MAX slots: every set row is among them, or the last slot
    # holds a row and the sweep reports the overflow
    overflow = got[SPARSE_MAX] >= 0
    assert overflow == (n_set > SPARSE_MAX)
    if not overflow:
        assert np.array_equal(np.sort(got[:SPARSE_MAX][got[:SPARSE_MAX] >= 0]), truth)


def test_sparse_rows_refuses_other_masks():
    import torch
    from concept_amd import commons
    with pytest.raises(ValueError):
        commons.sparse_rows(torch.zeros(4, dtype=torch.int8), SPARSE_MAX)
    with pytest.raises(ValueError):
        commons.sparse_rows(torch.zeros((2, 2), dtype=torch.bool), SPARSE_MAX)
