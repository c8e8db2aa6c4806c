"""TEST INFRASTRUCTURE: numpy restatement of the SU(3) heatbath / overrelaxation link update, written from the
formulas (include/l2q.h, "SU(3) heatbath and overrelaxation"), not from the kernel.  Reference layout
``x[nb, 4, T, X, Y, Z, 3, 3]`` complex128; the uniforms and the half-site order are the kernel's:
``u[nb, 3, 4 ntry + 2, V/2]``, half-site h = the h-th site with (t + x + y + z) & 1 == parity in lattice order."""
import numpy as np

from oracle import su3 as osu3

SUBGROUPS = ((0, 1), (0, 2), (1, 2))
TWO_PI = 2.0 * np.pi


def half_sites(L, parity):
    """flat site indices of one parity, in lattice order"""
    t, x, y, z = np.meshgrid(*[np.arange(n) for n in L], indexing='ij')
    return np.flatnonzero(((t + x + y + z) & 1).ravel() == parity)


def staple_mu(x, mu):
    """A_mu of oracle.su3.staples for one direction: [nb, T, X, Y, Z, 3, 3]"""
    a = np.zeros_like(x[:, mu])
    xm = x[:, mu]
    for nu in range(4):
        if nu == mu:
            continue
        xn = x[:, nu]
        xn_pmu = np.roll(xn, -1, axis=mu + 1)
        up = xn_pmu @ osu3.adj(np.roll(xm, -1, axis=nu + 1)) @ osu3.adj(xn)
        dn = (osu3.adj(np.roll(xn_pmu, +1, axis=nu + 1)) @ osu3.adj(np.roll(xm, +1, axis=nu + 1))
              @ np.roll(xn, +1, axis=nu + 1))
        a += up + dn
    return a


def qmul(a, b):
    """product of the 2 x 2 matrices a0 + i (a1 s1 + a2 s2 + a3 s3); a, b [4, ...]"""
    return np.stack([
        a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
        a[0] * b[1] + a[1] * b[0] - (a[2] * b[3] - a[3] * b[2]),
        a[0] * b[2] + a[2] * b[0] - (a[3] * b[1] - a[1] * b[3]),
        a[0] * b[3] + a[3] * b[0] - (a[1] * b[2] - a[2] * b[1])])


def qconj(a):
    return np.stack([a[0], -a[1], -a[2], -a[3]])


def embed(a, i, j):
    """[[a0 + i a3, a2 + i a1], [-a2 + i a1, a0 - i a3]] at rows / columns i, j of the 3 x 3 identity"""
    e = np.zeros(a.shape[1:] + (3, 3), dtype=np.complex128)
    e[..., 0, 0] = e[..., 1, 1] = e[..., 2, 2] = 1.0
    e[..., i, i] = a[0] + 1j * a[3]
    e[..., i, j] = a[2] + 1j * a[1]
    e[..., j, i] = -a[2] + 1j * a[1]
    e[..., j, j] = a[0] - 1j * a[3]
    return e


def su2_part(w, i, j):
    """r of the block (i, j) of w: Re tr(embed(a) w) = const + 2 (a r)_0"""
    return 0.5 * np.stack([(w[..., i, i] + w[..., j, j]).real, (w[..., i, j] + w[..., j, i]).imag,
                           (w[..., i, j] - w[..., j, i]).real, (w[..., i, i] - w[..., j, j]).imag])


def unit(r):
    """(k, r / k), r / k = (1, 0, 0, 0) where k is zero or not finite"""
    k = np.sqrt((r * r).sum(0))
    ok = (k > 0) & np.isfinite(k)
    e0 = np.zeros_like(r)
    e0[0] = 1.0
    with np.errstate(divide='ignore', invalid='ignore'):
        return k, np.where(ok, r / np.where(ok, k, 1.0), e0)


def kp_try(alpha, u1, u2, u3, u4):
    """one Kennedy-Pendleton proposal: (b0, accepted, |v4^2 - (1 - delta/2)|)"""
    v1, v2, v3, v4 = 1.0 - u1, 1.0 - u2, 1.0 - u3, 1.0 - u4
    with np.errstate(divide='ignore', invalid='ignore'):
        delta = -(np.log(v1) + np.cos(TWO_PI * v2) ** 2 * np.log(v3)) / alpha
        lim = 1.0 - 0.5 * delta
        return 1.0 - delta, v4 * v4 <= lim, np.abs(v4 * v4 - lim)


def kp_direction(b0, u5, u6):
    v5, v6 = 1.0 - u5, 1.0 - u6
    ct, phi = 1.0 - 2.0 * v5, TWO_PI * v6
    st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
    n = np.sqrt(np.maximum(0.0, 1.0 - b0 * b0))
    return np.stack([b0, n * st * np.cos(phi), n * st * np.sin(phi), n * ct])


def _update(x, mu, parity, beta=None, u=None, ntry=0):
    nb, L = x.shape[0], x.shape[2:6]
    V = int(np.prod(L))
    idx = half_sites(L, parity)
    a_st = staple_mu(x, mu).reshape(nb, V, 3, 3)[:, idx]
    lk = x[:, mu].reshape(nb, V, 3, 3)[:, idx].copy()
    fails = np.zeros(nb)
    margin = np.full((nb, 3, max(ntry, 1), idx.size), np.inf)
    for g, (i, j) in enumerate(SUBGROUPS):
        k, rh = unit(su2_part(lk @ a_st, i, j))
        rc = qconj(rh)
        if u is None:
            lk = embed(qmul(rc, rc), i, j) @ lk
            continue
        alpha = 2.0 * beta * k / 3.0
        done = np.zeros(k.shape, dtype=bool)
        b0 = np.ones(k.shape)
        for t in range(ntry):
            nb0, ok, m = kp_try(alpha, *(u[:, g, 4 * t + r] for r in range(4)))
            margin[:, g, t] = np.where(done, np.inf, m)
            take = ~done & ok
            b0 = np.where(take, nb0, b0)
            done |= take
        b = kp_direction(b0, u[:, g, 4 * ntry], u[:, g, 4 * ntry + 1])
        lk = np.where(done[..., None, None], embed(qmul(b, rc), i, j) @ lk, lk)
        fails += (~done).sum(1)
    out = x.copy()
    f = out[:, mu].reshape(nb, V, 3, 3)
    f[:, idx] = lk
    out[:, mu] = f.reshape(x[:, mu].shape)
    return out, fails, margin


def heatbath(x, beta, mu, parity, u, ntry):
    """-> (new links, fails [nb], margin [nb, 3, ntry, V/2]): margin = |v4^2 - (1 - delta/2)| of every try that was
    examined (inf for the tries after the accepted one)"""
    u = np.asarray(u)
    assert u.shape == (x.shape[0], 3, 4 * ntry + 2, int(np.prod(x.shape[2:6])) // 2), u.shape
    return _update(x, mu, parity, float(beta), u, int(ntry))


def overrelax(x, mu, parity):
    return _update(x, mu, parity)[0]


def heatbath_sweep(x, beta, ntry, rng, nover=0):
    """one sweep in the documented order (mu 0..3, parity 0, 1) with uniforms from a numpy Generator, then `nover`
    overrelaxation sweeps; -> (x, fails [nb])"""
    nb, vh = x.shape[0], int(np.prod(x.shape[2:6])) // 2
    fails = np.zeros(nb)
    for mu in range(4):
        for parity in (0, 1):
            x, f, _ = heatbath(x, beta, mu, parity, rng.random((nb, 3, 4 * ntry + 2, vh)), ntry)
            fails += f
    for _ in range(nover):
        for mu in range(4):
            for parity in (0, 1):
                x = overrelax(x, mu, parity)
    return x, fails


def random_links(rng, nb, L):
    """Haar-like random SU(3) links.  One closed-form projection of a Gaussian matrix is unitary to ~1e-11 only (its
    eigenvalue formula loses digits where two eigenvalues are close); the second one, applied to an almost unitary
    matrix, leaves ~3e-15, so that the 1e-12 group checks of the updates measure the update and not their input."""
    z = rng.normal(size=(nb, 4, *L, 3, 3)) + 1j * rng.normal(size=(nb, 4, *L, 3, 3))
    return osu3.project_su(osu3.project_su(z))
