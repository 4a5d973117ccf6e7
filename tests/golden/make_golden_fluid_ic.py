"""Golden vectors of the reference's fluid realisation (realize, realize_fluid, realize_grid:
ic.py:297-477, 708-764).

Run in the development container, one process per case (the reference keeps its parameters as
module globals):  python tests/golden/make_golden_fluid_ic.py
The reference is imported in pure-Python mode through oracle/refharness, its `ic` module the way
make_golden_lpt.py imports it.  realize(component, a) is driven whole on a fluid component of
Boltzmann order 1; CLASS is kept out by one replacement of a module attribute:
  ic.get_amplitudes   a lookup in the tables below (δ for variable 0, θ for variable 1)
and one wrapper that only records: generate_primordial_noise (the noise slab after the call).
Each fluid_ic_<case>_g<N>.npz holds the noise slab (its Nyquist planes, which the reference
leaves as it finds them, set to zero), both tables, ϱ_bar ('rho_bar'), w, w_eff, a and the
factor of J, and the grids ϱ ('rho') and J[0..2] without their ghost layers."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

A = 0.02
DELTA_RMS = 0.1

# name -> (realization_options, further parameters, grid sizes)
CASES = {
    'plain': ({}, {}, (8, 12, 16)),
    'nongauss': ({'nongaussianity': 0.5}, {}, (8, 12, 16)),
    'fixed_shift': ({}, {'primordial_amplitude_fixed': True,
                         'primordial_phase_shift': 'π'}, (8, 12)),
    'simple': ({}, {'primordial_noise_imprinting': "'simple'"}, (8, 12)),
}


def param_text(options, extra):
    lines = ['boxsize = 100.0*Mpc', 'H0 = 70*km/s/Mpc', 'Ωcdm = 0.25', 'Ωb = 0.05',
             f'a_begin = {A}', 'enable_class_background = False',
             f'realization_options = {options!r}']
    lines += [f'{key} = {val}' for key, val in extra.items()]
    return '\n'.join(lines) + '\n'


def tables(g, boxsize):
    """the smooth made-up spectrum of make_golden_lpt.py, scaled so that the expected rms of δ
    on this grid is DELTA_RMS (unit-variance noise: the variance of δ is the sum of amplitude²
    over the modes off the origin and the Nyquist planes): ϱ stays positive"""
    import numpy as np
    k2 = np.arange(3*(g//2 - 1)**2 + 1, dtype=np.float64)
    k = 2*np.pi/boxsize*np.sqrt(k2)
    amp = np.zeros_like(k2)
    amp[1:] = k[1:]**0.5/(1 + (k[1:]/0.25)**2)
    full = np.arange(-(g//2 - 1), g//2)
    ki, kj, kk = np.meshgrid(full, full, full, indexing='ij')
    amp *= DELTA_RMS/np.sqrt((amp[ki**2 + kj**2 + kk**2]**2).sum())
    amp_θ = -0.9*amp*(1 + 0.2*k/k[-1])
    return amp, amp_θ


def child(name, g):
    import importlib
    import numpy as np
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refharness'))
    from ref_import import load_reference
    options, extra, _ = CASES[name]
    text = param_text(options, extra)
    ref = load_reference(text, f'/tmp/concept_golden_work/fluid_ic_{name}_g{g}')
    commons, species = ref.commons, ref.species
    ic = importlib.import_module('ic')
    L = commons.boxsize
    amp, amp_θ = tables(g, L)
    recorded = {'calls': []}
    nyq = g//2

    def get_amplitudes(gridsize, component, a, a_next=-1, variable=0, multi_index=None, **kw):
        index = tuple(multi_index) if isinstance(multi_index, (tuple, list)) else (multi_index,)
        recorded['calls'].append((variable, index))
        return (amp_θ if variable == 1 else amp).copy()
    ic.get_amplitudes = get_amplitudes
    orig_noise = ic.generate_primordial_noise

    def noise(slab, fixed_amplitude=False, phase_shift=0):
        orig_noise(slab, fixed_amplitude, phase_shift)
        copy = np.array(slab).copy()
        copy[nyq, :, :] = 0
        copy[:, nyq, :] = 0
        copy[:, :, 2*nyq:] = 0
        recorded['noise'] = copy
    ic.generate_primordial_noise = noise

    comp = species.Component('matter', 'matter', gridsize=g, boltzmann_order=1)
    ic.realize(comp, A)
    assert recorded['calls'] == [(0, (0,)), (1, (0,)), (1, (1,)), (1, (2,))], recorded['calls']
    w, w_eff, ϱ_bar = comp.w(a=A), comp.w_eff(a=A), comp.ϱ_bar
    ϱ = np.array(comp.ϱ.grid_noghosts)[:g, :g, :g].copy()
    J = np.stack([np.array(comp.J[i].grid_noghosts)[:g, :g, :g].copy() for i in range(3)])
    δ = ϱ/ϱ_bar - 1
    print(f'{name} g{g}: δ rms {δ.std():.4f}, δ in [{δ.min():.4f}, {δ.max():.4f}], '
          f'max |J| {np.abs(J).max():.4g}')
    assert ϱ.min() > 0
    out = dict(param_text=text, gridsize=g, boxsize=L, a=A, rho_bar=ϱ_bar, w=w, w_eff=w_eff,
               J_factor=A**(1 - 3*w_eff)*ϱ_bar*(1 + w),
               nongaussianity=float(options.get('nongaussianity', 0.0)),
               amplitudes=amp, amplitudes_θ=amp_θ, noise=recorded['noise'], rho=ϱ, J=J)
    np.savez_compressed(os.path.join(HERE, f'fluid_ic_{name}_g{g}.npz'), **out)
    print('wrote', f'fluid_ic_{name}_g{g}', {k: getattr(v, 'shape', v) for k, v in out.items()
                                              if k != 'param_text'})


def main():
    if len(sys.argv) > 1:
        child(sys.argv[1], int(sys.argv[2]))
        return
    for name, (_, _, gridsizes) in CASES.items():
        for g in gridsizes:
            print('===', name, g, flush=True)
            log = f'/tmp/concept_golden_fluid_ic_{name}_g{g}.log'
            with open(log, 'w') as f:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(g)],
                                   stdout=f, stderr=subprocess.STDOUT)
            print('\n'.join(open(log).read().splitlines()[-3:]))
            if r.returncode:
                sys.exit(f'case {name} g{g} failed, see {log}')


if __name__ == '__main__':
    main()
