"""Golden vectors of the reference's power spectrum (analysis.py:70-93, 118-579, 856-914).

Run in the development container, one process per case (the reference keeps its parameters as
module globals):  python tests/golden/make_golden_powerspec.py
The reference is imported in pure-Python mode through oracle/refharness/ref_import.  Its
analysis module imports graphics, ic and linear, which need CLASS and matplotlib: those three
are stubbed here (with get_output_declarations, the one function the power spectrum uses,
taken from the reference's graphics.py source).  Per case: the inputs, k2_max,
k_bin_indices, k_bin_centers, n_modes, power and σ of every 'data' declaration."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

CASES = {
    # (a) the defaults: PCS, bcc, deconvolved, k_max = 'Nyquist'; clustered 16³ on 32³
    'powerspec_a_defaults': dict(
        boxsize=100.0, components=[('matter', 16**3, None)], options="", clustered=True),
    # (b) CIC, no interlacing, k_max = 1.5 Nyquist, one bins-per-decade value
    'powerspec_b_cic': dict(
        boxsize=80.0, components=[('matter', 16**3, None)],
        options="""powerspec_options = {'interpolation': 'CIC', 'interlace': False,
                     'k_max': '1.5*Nyquist', 'bins per decade': 12}
""", clustered=True),
    # (c) two particle components, upstream 16 and 24 on a global 24: per component and 'all'
    'powerspec_c_multigrid': dict(
        boxsize=90.0, components=[('light', 8**3, None), ('heavy', 12**3, None)],
        options="""powerspec_options = {'upstream gridsize': {'light': 16, 'heavy': 24},
                     'global gridsize': 24}
powerspec_select = {'all': True, 'all combinations': True}
""", clustered=True),
    # (d) a fluid and particles, combined
    'powerspec_d_fluid': dict(
        boxsize=70.0, components=[('matter', 8**3, None), ('fluid', None, 16)],
        options="""powerspec_options = {'gridsize': 16}
powerspec_select = {'all combinations': True}
""", clustered=False),
}


def param_text(cfg):
    return f"""
boxsize = {cfg['boxsize']!r}*Mpc
H0 = 70*km/s/Mpc
Ωcdm = 0.25
Ωb = 0.05
a_begin = 0.5
enable_class_background = False
{cfg['options']}
"""


def _stub_modules(ref_src):
    """graphics / ic / linear stand-ins for `import analysis`"""
    import re
    import types
    import commons
    graphics = types.ModuleType('graphics')
    src = open(os.path.join(ref_src, 'graphics.py'), encoding='utf-8').read()
    m = re.search(r'\n(@cython\.header\([^@]*?\)\ndef get_output_declarations.*?)\n# Cache used',
                  src, re.S)
    ns = dict(vars(commons))
    exec(m.group(1), ns)
    graphics.get_output_declarations = ns['get_output_declarations']
    ns['output_declarations_cache'] = {}
    def nothing(*a, **k):
        return None
    graphics.plot_powerspec = graphics.plot_bispec = nothing
    ic = types.ModuleType('ic')
    ic.realize = nothing
    linear = types.ModuleType('linear')
    for fname in ('compute_cosmo', 'get_linear_powerspec', 'get_treelevel_bispec',
                  'get_linear_component'):
        setattr(linear, fname, nothing)
    for mod in (graphics, ic, linear):
        mod.__file__ = os.path.abspath(__file__)
    sys.modules.update(graphics=graphics, ic=ic, linear=linear)


def child(name):
    import numpy as np
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refharness'))
    from ref_import import REFERENCE, load_reference
    cfg = CASES[name]
    ref = load_reference(param_text(cfg), f'/tmp/concept_golden_work/{name}')
    commons, species = ref.commons, ref.species
    _stub_modules(f'{REFERENCE}/src')
    import analysis
    L = commons.boxsize
    rng = np.random.default_rng(7 + len(name))
    out = dict(boxsize=L, a=commons.universals.a, param=param_text(cfg))
    comps = []
    for ci, (cname, N, gs) in enumerate(cfg['components']):
        if N is not None:
            n = round(N**(1/3))
            q = (np.arange(n) + 0.5)*L/n
            pos = np.stack(np.meshgrid(q, q, q, indexing='ij'), -1).reshape(-1, 3)
            if cfg['clustered']:
                # a few clumps on top of a displaced lattice
                centres = rng.uniform(0, L, (4, 3))
                pull = rng.integers(0, 4, len(pos))
                pos = pos + 0.35*(centres[pull] - pos) + rng.normal(0, 0.02*L, pos.shape)
            else:
                pos = pos + rng.normal(0, 0.05*L/n, pos.shape)
            pos = np.mod(pos, L)
            mass = commons.ρ_mbar*L**3/N*(1.0 + 0.3*ci)
            comp = species.Component(cname, 'matter', N=N, mass=mass)
            for d, s_ in enumerate('xyz'):
                comp.populate(np.ascontiguousarray(pos[:, d]), 'pos' + s_)
                comp.populate(np.zeros(N), 'mom' + s_)
            out[f'{cname}_pos'] = pos
            out[f'{cname}_mass'] = mass
            out[f'{cname}_N'] = N
        else:
            comp = species.Component(cname, 'matter', gridsize=gs, boltzmann_order=1)
            rho = commons.ρ_mbar*0.4*(1 + 0.3*rng.normal(size=(gs, gs, gs)))
            comp.populate(np.ascontiguousarray(rho), 'ϱ')
            out[f'{cname}_rho'] = rho
            out[f'{cname}_gridsize'] = gs
        out[f'{cname}_upstream'] = comp.powerspec_upstream_gridsize
        comps.append(comp)
    out['component_names'] = np.array([c[0] for c in cfg['components']])
    declarations = [d for d in analysis.get_powerspec_declarations(comps) if d.do_data]
    out['n_declarations'] = len(declarations)
    for i, d in enumerate(declarations):
        analysis.compute_powerspec(d)
        out[f'd{i}_components'] = np.array([c.name for c in d.components])
        out[f'd{i}_gridsize'] = d.gridsize
        out[f'd{i}_k2_max'] = d.k2_max
        out[f'd{i}_k_bin_indices'] = np.asarray(d.k_bin_indices).astype(np.int32)
        out[f'd{i}_k_bin_centers'] = np.asarray(d.k_bin_centers)
        out[f'd{i}_n_modes'] = np.asarray(d.n_modes)
        out[f'd{i}_power'] = np.asarray(d.power)
        out[f'd{i}_sigma'] = analysis.compute_powerspec_σ(d)
        out[f'd{i}_tophat'] = d.tophat
        out[f'd{i}_interpolation'] = d.interpolation
        out[f'd{i}_interlace'] = str(d.interlace)
        out[f'd{i}_k_max'] = str(d.k_max)
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
    print('wrote', name, {k: getattr(v, 'shape', v) for k, v in out.items() if k != 'param'})


def main():
    if len(sys.argv) > 1 and sys.argv[1] in CASES:
        child(sys.argv[1])
        return
    for name in CASES:
        print('===', name, flush=True)
        log = f'/tmp/concept_golden_{name}.log'
        with open(log, 'w') as f:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), name], stdout=f,
                               stderr=subprocess.STDOUT)
        print('\n'.join(open(log).read().splitlines()[-3:]))
        if r.returncode:
            sys.exit(f'case {name} failed, see {log}')


if __name__ == '__main__':
    main()
