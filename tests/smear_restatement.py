"""TEST INFRASTRUCTURE: numpy restatement of APE and HYP link smearing, vectorised over sites with `np.roll` shifts and
written from the formulas (include/l2q.h, "SU(3) APE and HYP link smearing"), not from the kernels.  Reference layout
``x[nb, 4, T, X, Y, Z, 3, 3]`` complex128; a decorated field is a dict ``{(mu, o): field[nb, T, X, Y, Z, 3, 3]}`` over the
12 ordered pairs mu != o; the APE directions D are the 4-bit set of the kernels (bit mu = direction mu).

The projection is a parameter: `oracle.su3.project_su` (the closed form the kernels restate) by default, or
`project_svd`, the same map by `numpy.linalg.svd` (polar factor, then the determinant phase), used only as a yardstick
for how far rounding in the closed form can move a result.  Every pre-projection matrix of every level and iteration
is checked against the input rule: condition number <= MAX_COND (the closed form loses accuracy beyond it), over all
links -- none is left out.  `stats`, when given, collects the worst condition number under 'cond'."""
import numpy as np

from oracle import su3 as osu3
from su3_truth import MAX_COND

PAIRS = [(mu, o) for mu in range(4) for o in range(4) if o != mu]        # the order of a native decorated field
APE_MASKS = [15, 14, 13, 11, 7, 6]               # 4D, the spatial masks of time_dir 0, 1, 2, 3, and one pair (x, y)
HYP_ALPHAS = (0.75, 0.6, 0.3)


def dirs(D):
    return [mu for mu in range(4) if (D >> mu) & 1]


def spatial(time_dir):
    return 15 & ~(1 << time_dir)


def sh(f, mu, n):
    """f(x + n mu) for a site field f[nb, T, X, Y, Z, ...]"""
    return np.roll(f, -n, axis=mu + 1)


def staples(a, b, mu, nu):
    """S_nu[A, B](x) = A(x) B(x+nu) A(x+mu)^H + A(x-nu)^H B(x-nu) A(x-nu+mu) for the side field a (direction nu) and the
    forward field b (direction mu)"""
    up = a @ sh(b, nu, 1) @ osu3.adj(sh(a, mu, 1))
    down = sh(osu3.adj(a) @ b @ sh(a, mu, 1), nu, -1)
    return up + down


def project_svd(m):
    """the unitary polar factor of m with the phase of its determinant divided out, by numpy's SVD"""
    u, _, vh = np.linalg.svd(m)
    w = u @ vh
    d = np.linalg.det(w)
    return w * np.exp(-1j * np.angle(d) / 3.0)[..., None, None]


def blend(u, s, alpha, nstaples, proj, stats):
    """Proj[(1 - alpha) u + (alpha / nstaples) s], the input rule checked on every matrix"""
    m = (1.0 - alpha) * u + (alpha / nstaples) * s
    sv = np.linalg.svd(m, compute_uv=False)
    cond = float((sv[..., 0] / sv[..., -1]).max())
    assert cond <= MAX_COND, f'input rule: a pre-projection matrix has condition number {cond:.3g} > {MAX_COND}'
    if stats is not None:
        stats['cond'] = max(stats.get('cond', 0.0), cond)
    return proj(m)


def ape_step(x, alpha, D, proj=osu3.project_su, stats=None):
    d = dirs(D)
    n = len(d) - 1
    out = x.copy()
    for mu in d:
        s = sum(staples(x[:, nu], x[:, mu], mu, nu) for nu in d if nu != mu)
        out[:, mu] = blend(x[:, mu], s, alpha, 2 * n, proj, stats)
    return out


def ape(x, alpha, D, nsteps, proj=osu3.project_su, stats=None):
    for _ in range(nsteps):
        x = ape_step(x, alpha, D, proj, stats)
    return x


def hyp_level1(x, alpha3, proj=osu3.project_su, stats=None):
    """B1[mu][eta] = Proj[(1 - alpha3) U_mu + (alpha3 / 2) S_eta[U_eta, U_mu]]"""
    return {(mu, eta): blend(x[:, mu], staples(x[:, eta], x[:, mu], mu, eta), alpha3, 2, proj, stats)
            for mu, eta in PAIRS}


def hyp_level2(x, b1, alpha2, proj=osu3.project_su, stats=None):
    """B2[mu][nu] = Proj[(1 - alpha2) U_mu + (alpha2 / 4) sum_{rho not in {mu, nu}} S_rho[B1[rho][eta], B1[mu][eta]]],
    eta = 6 - mu - nu - rho"""
    out = {}
    for mu, nu in PAIRS:
        s = sum(staples(b1[rho, 6 - mu - nu - rho], b1[mu, 6 - mu - nu - rho], mu, rho)
                for rho in range(4) if rho not in (mu, nu))
        out[mu, nu] = blend(x[:, mu], s, alpha2, 4, proj, stats)
    return out


def hyp_level3(x, b2, alpha1, proj=osu3.project_su, stats=None):
    """V_mu = Proj[(1 - alpha1) U_mu + (alpha1 / 6) sum_{nu != mu} S_nu[B2[nu][mu], B2[mu][nu]]]"""
    out = np.empty_like(x)
    for mu in range(4):
        s = sum(staples(b2[nu, mu], b2[mu, nu], mu, nu) for nu in range(4) if nu != mu)
        out[:, mu] = blend(x[:, mu], s, alpha1, 6, proj, stats)
    return out


def hyp_step(x, alphas=HYP_ALPHAS, proj=osu3.project_su, stats=None):
    a1, a2, a3 = alphas
    b1 = hyp_level1(x, a3, proj, stats)
    b2 = hyp_level2(x, b1, a2, proj, stats)
    return hyp_level3(x, b2, a1, proj, stats)


def hyp(x, alphas, nsteps, proj=osu3.project_su, stats=None):
    for _ in range(nsteps):
        x = hyp_step(x, alphas, proj, stats)
    return x


def dec_stack(b):
    """a decorated dict -> [nb, 4, 3, T, X, Y, Z, 3, 3] in the order of the native decorated field"""
    return np.stack([np.stack([b[mu, o] for o in range(4) if o != mu], 1) for mu in range(4)], 1)


def dec_dict(a):
    """the inverse of dec_stack"""
    return {(mu, o): a[:, mu, o - (o > mu)] for mu, o in PAIRS}


def yardsticks(x, ape_cases, hyp_alphas=HYP_ALPHAS, hyp_steps=1):
    """The largest element-wise deviation between the restatement with the closed-form projection and with the SVD
    projection, per operation, on the input x: {'ape': over ape_cases [(alpha, D, nsteps), ...] run end to end, 'hyp':
    hyp_steps HYP steps end to end, 'level1' / 'level2' / 'level3': each single level from the same (closed-form)
    inputs} and the worst condition number met under 'cond'."""
    st = {}
    out = {'ape': 0.0}
    for alpha, D, nsteps in ape_cases:
        out['ape'] = max(out['ape'], float(np.abs(ape(x, alpha, D, nsteps, stats=st)
                                                  - ape(x, alpha, D, nsteps, project_svd)).max()))
    out['hyp'] = float(np.abs(hyp(x, hyp_alphas, hyp_steps, stats=st) - hyp(x, hyp_alphas, hyp_steps, project_svd)).max())
    a1, a2, a3 = hyp_alphas
    b1 = hyp_level1(x, a3, stats=st)
    b2 = hyp_level2(x, b1, a2, stats=st)
    out['level1'] = float(np.abs(dec_stack(b1) - dec_stack(hyp_level1(x, a3, project_svd))).max())
    out['level2'] = float(np.abs(dec_stack(b2) - dec_stack(hyp_level2(x, b1, a2, project_svd))).max())
    out['level3'] = float(np.abs(hyp_level3(x, b2, a1) - hyp_level3(x, b2, a1, project_svd)).max())
    out['cond'] = st['cond']
    return out


# ------------------------------------------------------------------ the inputs and tolerances of the smearing tests
KERNEL_LATTICES = [(2, 2, 2, 2), (4, 2, 6, 2), (3, 4, 5, 2), (4, 1, 6, 2)]       # host emulation and GPU
GPU_LATTICES = KERNEL_LATTICES + [(4, 4, 4, 8), (4, 4, 4, 10)]                   # whole blocks; a partial last block
API_LATTICES = [(4, 4, 4, 4), (3, 4, 5, 2)]
AMP = 0.3
APE_CASES = [(0.7, 15)] + [(0.5, m) for m in APE_MASKS[1:]]                      # (alpha, mask) of the kernel tests
API_STEPS = (0, 1, 3)


def smooth_input(L, nb=3, amp=AMP):
    """the smooth links exp(i amp H) every smearing test of lattice L starts from (the input rule: Haar-random links
    reach condition numbers of 150-240 at HYP levels 2 / 3 and in the 4D APE step, these stay below 3)"""
    from gaugefix_restatement import smooth_links
    return smooth_links(np.random.default_rng(7000 + 1000 * L[0] + 100 * L[1] + 10 * L[2] + L[3]), nb, tuple(L), amp)


# Yardsticks: the largest element-wise deviation between this restatement run end to end with the closed-form projection
# and with the SVD projection, per operation, over the inputs above (`python tests/smear_restatement.py --measure` prints
# them; measured: ape 5.62e-15, hyp 5.25e-15, level1 5.54e-15, level2 5.55e-15, level3 5.08e-15 over GPU_LATTICES and
# API_LATTICES at one step, worst condition number 2.1; three steps end to end, as the interface tests iterate, give no
# more: ape 5.60e-15, hyp 5.00e-15, so the iterated comparisons use the same figures).  The kernels differ from numpy by fma
# contraction and summation order over up to 19 3x3 products per link: the tolerance is 32 x the yardstick and covers that
# and nothing else.  tests/test_smear_host.py measures the yardsticks of the small lattices again and holds them to these figures.
YARDSTICK = {'ape': 5.7e-15, 'hyp': 5.3e-15, 'level1': 5.6e-15, 'level2': 5.6e-15, 'level3': 5.1e-15}
TOL = {k: 32.0 * v for k, v in YARDSTICK.items()}


def measure():
    worst = {}
    for L in GPU_LATTICES + API_LATTICES[:1]:
        y = yardsticks(smooth_input(L), [(a, m, 1) for a, m in APE_CASES])
        print(L, {k: float(f'{v:.3g}') for k, v in y.items()})
        for k, v in y.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print('one step, worst:', {k: float(f'{v:.3g}') for k, v in worst.items()})
    worst = {}
    for L in API_LATTICES:
        x = smooth_input(L)
        for n in API_STEPS[1:]:
            y = yardsticks(x, [(0.5, spatial(0), n), (0.5, spatial(1), n), (0.7, 15, n)], hyp_steps=n)
            print(L, n, 'steps:', {k: float(f'{y[k]:.3g}') for k in ('ape', 'hyp', 'cond')})
            for k in ('ape', 'hyp', 'cond'):
                worst[k, n] = max(worst.get((k, n), 0.0), y[k])
    print('iterated, worst:', {k: float(f'{v:.3g}') for k, v in worst.items()})


if __name__ == '__main__':
    import sys
    if '--measure' in sys.argv:
        measure()
