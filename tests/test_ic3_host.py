"""Host side of 3LPT and Orszag dealiasing (concept_amd/ic.py), no GPU: the dealiasing size, the
term tables against the formulas in the reference's comments (ic.py:1554-1561, 1633-1639,
1711-1721, 1801-1808), the term evaluator's sequence of derivatives against the reference's own
(tests/golden/lpt3_*.npz, made by make_golden_lpt3.py), the refusals, the binding's new symbols."""
import glob
import os

import numpy as np
import pytest

from test_ic_host import FakeComponent

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(f)[5:-4] for f in glob.glob(os.path.join(GOLDEN, 'lpt3_*.npz')))


def test_the_golden_cases_are_all_there():
    names = {'3lpt', '3lpt_dealias', '2lpt_dealias', '3lpt_bcc2', '3lpt_dealias_vertex'}
    assert set(CASES) == {f'{name}_g{g}' for name in names for g in (8, 12)} | {'3lpt_dealias_g10'}


def test_dealias_gridsize():
    from concept_amd import ic
    assert [ic.dealias_gridsize(n) for n in (6, 8, 10, 12, 1024)] == [10, 12, 16, 18, 1536]


def coefficients(terms):
    """{sorted factors of a product: its signed coefficient}; the first term assigns"""
    out = {}
    for n, (output, operation, factor, pots) in enumerate(terms):
        assert (operation == '=') == (n == 0) and operation in ('=', '+=', '-=')
        assert len({output for output, *_ in terms}) == 1
        key = tuple(sorted(pots))
        assert key not in out
        out[key] = -factor if operation == '-=' else factor
    return out


def d1(*dims):
    return ('Φ1',) + tuple(sorted(dims))


def d2(*dims):
    return ('Φ2',) + tuple(sorted(dims))


def product(*pots):
    return tuple(sorted(pots))


def test_term_tables_are_the_formulas_of_the_reference():
    from concept_amd import ic
    # -Φ,₀₀Φ,₁₁ - Φ,₁₁Φ,₂₂ - Φ,₂₂Φ,₀₀ + Φ,₀₁² + Φ,₁₂² + Φ,₂₀²
    assert coefficients(ic.LPT_TERMS_2) == {
        product(d1(0, 0), d1(1, 1)): -1, product(d1(1, 1), d1(2, 2)): -1,
        product(d1(2, 2), d1(0, 0)): -1, product(d1(0, 1), d1(0, 1)): 1,
        product(d1(1, 2), d1(1, 2)): 1, product(d1(2, 0), d1(2, 0)): 1}
    # +Φ,₂₀²Φ,₁₁ - Φ,₁₁Φ,₂₂Φ,₀₀ + Φ,₀₀Φ,₁₂² - 2Φ,₁₂Φ,₂₀Φ,₀₁ + Φ,₀₁²Φ,₂₂
    assert coefficients(ic.LPT_TERMS_3A) == {
        product(d1(2, 0), d1(2, 0), d1(1, 1)): 1,
        product(d1(1, 1), d1(2, 2), d1(0, 0)): -1,
        product(d1(0, 0), d1(1, 2), d1(1, 2)): 1,
        product(d1(1, 2), d1(2, 0), d1(0, 1)): -2,
        product(d1(0, 1), d1(0, 1), d1(2, 2)): 1}
    # -½ Σ_{i≠j} Φ⁽¹⁾,ᵢᵢΦ⁽²⁾,ⱼⱼ + Σ_{i<j} Φ⁽²⁾,ᵢⱼΦ⁽¹⁾,ᵢⱼ
    expected = {product(d1(i, i), d2(j, j)): -0.5 for i in range(3) for j in range(3) if i != j}
    expected.update({product(d2(i, j), d1(i, j)): 1 for i in range(3) for j in range(i + 1, 3)})
    assert len(expected) == 9 and coefficients(ic.LPT_TERMS_3B) == expected
    # +Φ⁽²⁾,ⱼⱼΦ⁽¹⁾,ⱼₖ - Φ⁽¹⁾,ⱼₖΦ⁽²⁾,ₖₖ - Φ⁽¹⁾,ᵢⱼΦ⁽²⁾,ᵢₖ - Φ⁽¹⁾,ⱼⱼΦ⁽²⁾,ⱼₖ + Φ⁽²⁾,ⱼₖΦ⁽¹⁾,ₖₖ + Φ⁽²⁾,ᵢⱼΦ⁽¹⁾,ᵢₖ
    for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        assert coefficients(ic.lpt_terms_3c(i)) == {
            product(d2(j, j), d1(j, k)): 1, product(d1(j, k), d2(k, k)): -1,
            product(d1(i, j), d2(i, k)): -1, product(d1(j, j), d2(j, k)): -1,
            product(d2(j, k), d1(k, k)): 1, product(d2(i, j), d1(i, k)): 1}
    # 38 product terms for a 3LPT realisation
    orders = ic.lpt_orders(3)
    assert [name for name, *_ in orders] == ['Φ2', 'Φ3a', 'Φ3b', 'A3c0', 'A3c1', 'A3c2']
    assert sum(len(terms) for _, terms, *_ in orders) == 6 + 5 + 9 + 3*6 == 38
    assert [name for name, *_ in ic.lpt_orders(2)] == ['Φ2'] and ic.lpt_orders(1) == []
    # Ψ⁽³ᶜ⁾ = ∇ × A: Ψⱼ = ε_{jki} ∂ₖAᵢ summed over the three Aᵢ
    curl = {}
    for i, (_, _, _, _, _, passes) in enumerate(orders[3:]):
        for dim_diff, sign, dim in passes:
            curl[dim, dim_diff, i] = sign
    assert curl == {(0, 1, 2): 1, (0, 2, 1): -1, (1, 2, 0): 1, (1, 0, 2): -1, (2, 0, 1): 1,
                    (2, 1, 0): -1}
    # the factors that divide the growth factors
    g = {'D1': 3.0, 'D2': 5.0}
    assert [den(g) for _, _, _, den, *_ in orders] == [9, 27, 15, 15, 15, 15]
    assert [(D, f) for _, _, D, _, f, _ in orders] == [
        ('D2', 'f2'), ('D3a', 'f3a'), ('D3b', 'f3b')] + [('D3c', 'f3c')]*3


class Recorder:
    """stands in for a mesh: keeps what is asked of it"""
    def __init__(self, name, gridsize, log):
        self.name, self.gridsize, self.log = name, gridsize, log

    def lpt_diff(self, source, dim0, dim1=-1, factor=1.0):
        self.log.append(('diff', source.name, dim0, dim1, float(factor), False, self.name))

    def lpt_diff_enlarge(self, source, dim0, dim1=-1, factor=1.0):
        assert self.gridsize > source.gridsize
        self.log.append(('diff', source.name, dim0, dim1, float(factor), True, self.name))

    def lpt_product(self, a, b, operation='=', factor=1.0):
        assert a.gridsize == b.gridsize == self.gridsize
        self.log.append(('product', self.name, a.name, b.name, operation, factor))

    def lpt_shrink_accumulate(self, source, operation='=', factor=1.0):
        assert source.gridsize > self.gridsize
        self.log.append(('shrink', self.name, source.name, operation, factor))

    def lpt_dealias_cube(self, gridsize_small):
        self.log.append(('cube', self.name, gridsize_small))

    def lpt_potential(self, noise, amplitudes=None, shift=(0, 0, 0), factor=1.0):
        assert noise is self and amplitudes is None
        self.log.append(('potential', self.name, factor))

    def fft_forward(self):
        self.log.append(('forward', self.name))

    def poisson_backward(self):
        self.log.append(('backward', self.name))

    def lpt_displace(self, pos, mom, dim, pos_factor, mom_factor, index_bgn=0):
        self.log.append(('displace', self.name, dim, pos_factor, mom_factor))


def run_recorded(g):
    from concept_amd import commons, ic
    p = commons.load_params(str(g['param_text']))
    options = ic.realization_options(FakeComponent(p, 8))
    lpt, dealias = int(options['lpt']), bool(options['dealias'])
    n = int(g['gridsize'])
    m = ic.dealias_gridsize(n)
    log = []
    potentials = {name: Recorder(name, n, log) for name in ('Φ1', 'Φ2', 'Φ3')}
    tmps = [Recorder(f'tmp{i}', n, log) for i in range(2)]
    big = [Recorder(f'tmp{i} dealias', m, log) for i in range(2)] if dealias else None
    terms = ic.LptTerms(potentials, tmps, big)
    growth = dict(zip(g['growth_keys'].tolist(), g['growth_values'].tolist()))
    seen = []
    ic.carryout_lpt(ic.lpt_orders(lpt), terms, growth, float(g['a']), float(g['hubble']),
                    float(g['mass']), on_potential=lambda name, mesh, f: seen.append((name, f)))
    return log, seen, (lpt, dealias, bool(options['backscale']), n, m)


@pytest.mark.parametrize('case', CASES)
def test_the_evaluator_issues_the_reference_sequence_of_derivatives(golden, case):
    """which covers the reuse of the temporary grids' contents: a derivative made again, or
    one reused that is no longer there, changes the sequence or its length"""
    g = golden('lpt3_' + case)
    log, seen, (lpt, dealias, backscale, n, m) = run_recorded(g)
    ref = list(zip(g['diff_potential'].tolist(), g['diff_dims'][:, 0].tolist(),
                   g['diff_dims'][:, 1].tolist(), g['diff_factor'].tolist(),
                   g['diff_enlarged'].tolist()))
    # 1LPT first: three first derivatives of Φ⁽¹⁾ per variable (ic.py:1504-1505)
    n_first = 3*(1 if backscale else 2)
    assert ref[:n_first] == [('Φ1', i, -1, 1.0, False) for i in range(3)]*(n_first//3)
    got = [entry[1:6] for entry in log if entry[0] == 'diff']
    assert got == ref[n_first:]
    assert len(got) == {2: 10, 3: 68}[lpt]
    # the derivatives of the products are enlarged, those of the displacements never
    for _, potential, dim0, dim1, factor, enlarged, where in log_of(log, 'diff'):
        assert enlarged == (dealias and dim1 >= 0)
        assert where.endswith('dealias') == enlarged
    # every potential gets the reference's factor
    names = ['Φ2'] + ['Φ3a', 'Φ3b', 'A3c0', 'A3c1', 'A3c2']*(lpt == 3)
    keys = ['Phi2'] + ['Phi3a', 'Phi3b', 'A3c0', 'A3c1', 'A3c2']*(lpt == 3)
    assert [name for name, _ in seen] == names
    for (name, factor), key in zip(seen, keys):
        assert factor == float(g[key + '_factor']), name
    # the passes: a forward transform of the potential only without dealiasing; with it, one
    # shrink per term, one cube per triple product, and M⁻³ once per cube in the factor
    n_terms = {2: 6, 3: 38}[lpt]
    n_triple = {2: 0, 3: 5}[lpt]
    forwards = [entry[1] for entry in log_of(log, 'forward')]
    shrinks = log_of(log, 'shrink')
    if dealias:
        assert len(shrinks) == n_terms and len(log_of(log, 'cube')) == n_triple
        assert all(entry[2] == n for entry in log_of(log, 'cube'))
        assert all(name.endswith('dealias') for name in forwards)
        assert len(forwards) == n_terms + n_triple
        assert sorted(abs(entry[4]) for entry in shrinks if abs(entry[4]) < 0.1) == sorted(
            [float(m)**-3]*4 + [2*float(m)**-3])[:n_triple]
        assert all(entry[1].endswith('dealias') for entry in log_of(log, 'product'))
    else:
        assert not shrinks and not log_of(log, 'cube')
        assert forwards == ['Φ2'] + ['Φ3']*5*(lpt == 3)
        assert len(log_of(log, 'product')) == n_terms + n_triple
    assert len(log_of(log, 'displace')) == {2: 3, 3: 3 + 3 + 3 + 3*2}[lpt]


def log_of(log, kind):
    return [entry for entry in log if entry[0] == kind]


def test_a_square_reads_one_grid_twice_and_its_copy_is_never_made(golden):
    """Φ,₀₁² is lpt_product(x, x); the grid the reference copies it into is the one read"""
    log, _, _ = run_recorded(golden('lpt3_3lpt_g8'))
    squares = [entry for entry in log_of(log, 'product') if entry[2] == entry[3]]
    assert len(squares) == 3 + 2  # Φ,₀₁², Φ,₁₂², Φ,₂₀² of 2LPT; Φ,₂₀²Φ,₁₁ and Φ,₀₁²Φ,₂₂ of 3a
    # Φ,₂₀² of 2LPT is what 3a begins with: its derivative is not made a second time
    diffs = [entry[1:4] for entry in log_of(log, 'diff')]
    assert diffs[6] == ('Φ1', 0, 2) and diffs[10] == ('Φ1', 1, 1)


def test_growth_factors_are_refused_by_name():
    from concept_amd import commons, ic
    from concept_amd.lib import ConceptGPUError
    amp = np.zeros(28)
    p = commons.load_params({'boxsize': 10.0,
                             'realization_options': {'lpt': 3, 'backscale': True}})
    c = FakeComponent(p, 512)
    growth = {'D1': 0.02, 'f1': 1.0, 'D2': -1e-4, 'f2': 2.0, 'D3a': 1e-6, 'f3b': 3.0}
    with pytest.raises(ConceptGPUError) as e:
        ic.realize_particles(c, 0.02, amp, amp, growth, extended=True)
    assert str(e.value) == ("matter: growth factors ['f3a', 'D3b', 'D3c', 'f3c'] are needed")
    with pytest.raises(ConceptGPUError) as e:
        ic.realize(c, 0.02, amp, amp, growth_factors={'D1': 0.02}, extended=True)
    assert str(e.value) == ("matter: growth factors ['f1', 'D2', 'f2', 'D3a', 'f3a', 'D3b', "
                            "'f3b', 'D3c', 'f3c'] are needed")


def test_extended_refuses_4lpt_and_keeps_the_other_refusals():
    from concept_amd import commons, ic
    from concept_amd.lib import ConceptGPUError
    amp = np.zeros(28)

    def refuse(message, extended, n=512, comp=None, **options):
        p = commons.load_params({'boxsize': 10.0, 'realization_options': options})
        c = FakeComponent(p, n, **(comp or {}))
        with pytest.raises(ConceptGPUError) as e:
            ic.realize_particles(c, 0.02, amp, amp, extended=extended)
        assert str(e.value) == message
    refuse('matter: realize_particles() called with attempted 4LPT, though only 1LPT, 2LPT and '
           '3LPT are implemented', True, lpt=4)
    refuse('matter: realization_options["nongaussianity"] = 0.5: non-Gaussian initial '
           'conditions are not implemented', True, lpt=3, nongaussianity=0.5)
    refuse('matter: Can only realize particles using the primordial structure, not "nonlinear"',
           True, dealias=True, structure='non-linear')
    refuse('matter: realize_particles() called with a non-particle component (fluid realisation '
           'is not implemented)', True, lpt=3, comp={'representation': 'fluid'})
    refuse('Cannot initialize particle component matter with N = 1536 on a lattice, as neither '
           'of {N, N/2, N/4} is a cubic number', True, lpt=3, dealias=True, n=1536)
    refuse('matter: realize_particles() with an active comm process group: multi-GPU '
           'realisation is not implemented', True, lpt=3, comp={'nprocs': 2})
    # without the keyword, and with it set to False, nothing has changed
    refuse('matter: realization_options["lpt"] = 3: 3LPT is not implemented (1LPT and 2LPT are)',
           False, lpt=3)
    refuse('matter: realization_options["dealias"]: Orszag dealiasing of the LPT products is '
           'not implemented', False, lpt=2, dealias=True)
    refuse('matter: realize_particles() called with attempted 4LPT, though only 1LPT and 2LPT '
           'are implemented', False, lpt=4)


def test_the_new_symbols_are_bound_and_declared():
    from concept_amd import lib
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, 'include',
                               'concept_gpu.h'), encoding='utf-8').read()
    for name in ('cg_lpt_diff_enlarge', 'cg_lpt_dealias_cube', 'cg_lpt_shrink_accumulate'):
        assert name in lib.SYMBOLS and hasattr(lib.raw(), name)
        assert f'int {name}(' in header
