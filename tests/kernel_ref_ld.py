"""Extended-precision reference kernels, derived rounding bounds and input families for the tests
of kernel evaluation outside the unit cube (tests/test_kernel_ref_cpu.py,
tests/test_gpu_kernel_domain.py).  A helper module: nothing here is collected as a test.

A description is a list of terms in `+` order, a term being a kind or a list of kinds (its factors
in `*` order), as in tests/test_product_cpu.py: `[[SE, PER], WN]` is `SE * PER + WN`.

Reference
---------
`kernel_ld` / `kernel_grad_ld` evaluate include/gpr_hip.h's definitions in numpy.longdouble (x87
extended, eps 2^-63; anything coarser is refused) from the exact float64 x and hp, promoted before
any arithmetic: the difference form D = sum_k (l_k (x_k - x'_k))^2 (l_k x_k - l_k x'_k with the
common factor taken out: the same number, without the cancellation of two products rounded at
2^-64 of |l x|), sum_k (2 l_k sin(pi (x_k - x'_k) / p_k))^2 for Periodic, eps once per term on a
same-object diagonal, the first WhiteNoise's sigma_n^2 in the GPR_SELF form only.

Bounds (u = 2^-53)
------------------
Features.  The library scales once per call: s = fl(x l) (error <= u |s| per feature); a Periodic
part embeds f = [l cos(2 pi x / p) | l sin(2 pi x / p)] by sincospi(fl(2 x / p)): the quotient is
off by u |2x/p|, i.e. pi u |2x/p| in the angle, sincospi and the product by l round once each, so
each of the 2d features is off by at most df = l (pi u |2x/p| + 2u).  Write e_ak for that feature
error (u |s_ak| or df_ak), D for the distance of the computed features and Delta = s_a - s_b.

Difference form (GPR_KBUILD_EXACT=1, gpr_kernel_grad, the fused MLL gradient):
    D^ = sum_k fl(s_ak - s_bk)^2 by an fma chain.
  * the features' own errors move Delta_k by at most e_ak + e_bk:   2 sum_k |Delta_k| (e_ak + e_bk)
  * fl(s_ak - s_bk) is off by u |Delta_k|, squared: 2u Delta_k^2;   2u D
  * de fused multiply-adds, each rounding a partial sum <= D:        de u D
    B_diff = 2 sum_k |Delta_k| (e_ak + e_bk) + (de + 2) u D
  (The fused MLL gradient forms sum_k fl(l_k^2) fl(x_ak - x_bk)^2 on raw x with four partial sums:
  (ceil(d/4) + 6) u D, which B_diff covers from d = 3 on, its first term being >= 2u D.)

Gram form (the default): y = fl(s - c) with c the centre (the fp64 mean of the first min(n, 2048)
row points' features, also for the columns of a cross matrix), -D^ = fl(-|y_a|^2 - |y_b|^2) +
sum_k (2 y_ak) y_bk accumulated on the matrix pipe.  With N = |y_a|^2 + |y_b|^2:
  * fl(s - c) is off by u |y|, which moves y_ak - y_bk by u (|y_ak| + |y_bk|):
    2u sum |Delta_k| (|y_ak| + |y_bk|) <= u (D + 2N)  (the u D is inside B_diff's 2u D)    2 u N
  * each norm is an fma chain of de terms:                                                  de u N
  * the start value -|y_a|^2 - |y_b|^2 rounds once:                                            u N
  * de accumulations in any order, each rounding a partial sum <= N + sum |2 y_a y_b| <= 2N: 2 de u N
  * products rounded on their own where the accumulation is not fused: sum u |2 y_a y_b| <=    u N
    B_gram = B_diff + (3 de + 4) u N
  The centre is whatever the device's tree sum gives; the bound uses the fp64 mean and widens every
  |y_k| by cnt u max|s_k|, the worst case of any summation order.  A part that is not Periodic in a
  description with a Periodic part carries d zero features: they add exact zeros, so de = d there.

Element.  A factor's value k = sigma^2 f(D) moves by at most W B for a distance error B, W = -dk/dD
taken at max(D - B, 0) (every profile's W decreases in D, so this is the mean-value bound, and the
clamp sqrt(max(D, 0)) of the Matern profiles only shortens the path).  The table exponential of
kexp.hpp, steps as listed there, in units of u relative to the value:
    T[j] = 2^(j/256) rounded once from extended precision                  1
    expm1 by a degree-4 polynomial, |r| <= ln2/512: r^5/120 <= 3.8e-17      0.35
    the reduction residue: n L1 exact for |n| < 2^19 (D <= 800: n <= 295465), the second
      Cody-Waite step rounds r once (u |r| <= 1.4e-3 u) and L2's own rounding is n L2 u < 3e-7 u;
      the polynomial's roundings enter times r^2                            < 0.01
    fma(t, q, t)                                                           1
  E_EXP = 2.5 covers their sum 2.36.  The table is filled as fl(fl(sigma sigma) T[j]): two more
  roundings whenever sigma^2 is not a power of two, E_S2 = 2, so E = E_EXP + E_S2 = 4.5 per factor.
  (That is above 4 by the sigma^2 prefactor alone; DESIGN 3.5.1 says so.)
  The library exponential of the difference-form fallback kernels is within 1 ulp = 2u, times
  fl(sigma sigma) and the product: 4 <= E.  ldexp rounds once more into the subnormals, and a
  Matern profile multiplies by its polynomial P afterwards: (P + 1) 2^-1074, two subnormal steps
  for SquaredExp.  Matern also rounds a = sqrt(3|5), sqrt(D) and their product
  (3u in a r, i.e. 3u a r |dk/d(a r)|) and its polynomial and final product (4u).
    |dk| <= W(max(D - B, 0)) B + E u k + (P + 1) 2^-1074  [+ u (4 k + 3 a r |dk/d(a r)|)]
  A product of F factors: sum over factors of that times the other factors' values (taken with
  their own bounds added), plus (F - 1) (u T + 2^-1074) for the products; a sum of terms, eps and
  the noise: u |K| per addition.
"""
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1.1e-19, "numpy.longdouble is not x87 extended precision here"

SE, WN, M32, M52, PER = "SE", "WN", "M32", "M52", "PER"
EPS = 1e-8
U = 2.0 ** -53
TINY = LD(2.0) ** -1074
E_EXP = 2.5
E_S2 = 2.0
E_TOT = E_EXP + E_S2
CENTER_PTS = 2048
NORTH_STAR = 1e-8
PI_LD = LD("3.14159265358979323846264338327950288")
LN2_LD = LD("0.693147180559945309417232121458176568")
CROSS, SELF, SAME_OBJECT = 0, 1, 2
_INFL = 1.0 + 1e-9  # the bounds themselves are evaluated in floating point


# ---------------------------------------------------------------------------------------
# descriptions
# ---------------------------------------------------------------------------------------
def terms(desc):
    return [list(t) if isinstance(t, (list, tuple)) else [t] for t in desc]


def flat(desc):
    return [f for t in terms(desc) for f in t]


def width(kind, d):
    return 1 if kind == WN else 2 * d + 1 if kind == PER else d + 1


def split_hp(desc, hp, d):
    """per term the list of (kind, hp vector) of its factors"""
    hp = np.asarray(hp, dtype=np.float64)
    assert sum(width(k, d) for k in flat(desc)) == len(hp), "Parameter size mismatch."
    out, c = [], 0
    for t in terms(desc):
        fs = []
        for k in t:
            fs.append((k, hp[c:c + width(k, d)]))
            c += width(k, d)
        out.append(fs)
    return out


def same_mode(xp, x, same):
    if same is not None:
        return same
    return SELF if xp is None else SAME_OBJECT if xp is x else CROSS


# ---------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------
def factor_dist_ld(kind, h, x, xq):
    d = x.shape[0]
    X, XQ = np.asarray(x, dtype=LD), np.asarray(xq, dtype=LD)
    l = np.asarray(h[1:d + 1], dtype=LD)
    D = np.zeros((x.shape[1], xq.shape[1]), dtype=LD)
    for k in range(d):
        r = X[k][:, None] - XQ[k][None, :]
        if kind == PER:
            t = r / LD(h[d + 1 + k])
            t = t - np.rint(t)  # sin(pi t) has period 2 and sin^2 period 1: only the square is used
            c = LD(2) * l[k] * np.sin(PI_LD * t)
        else:
            c = l[k] * r
        D += c * c
    return D


def profile_ld(kind, D):
    """(f, w, P, ar, |df/d(ar)|): k = sigma^2 f, W = sigma^2 w = -dk/dD, P the polynomial"""
    if kind in (SE, PER):
        e = np.exp(-D)
        return e, e, LD(1), None, None
    a = np.sqrt(LD(3 if kind == M32 else 5))
    ar = a * np.sqrt(D)
    e = np.exp(-ar)
    if kind == M32:
        return (LD(1) + ar) * e, LD(1.5) * e, LD(1) + ar, ar, ar * e
    P = LD(1) + ar + ar * ar / LD(3)
    return P * e, (LD(5) / LD(6)) * (LD(1) + ar) * e, P, ar, (ar / LD(3)) * (LD(1) + ar) * e


def neg_dw_ld(kind, D):
    """-dw/dD of the profile (SE, PER, M52; Matern-3/2's W has no derivative at D = 0)"""
    if kind in (SE, PER):
        return np.exp(-D)
    assert kind == M52
    return (LD(25) / LD(12)) * np.exp(-np.sqrt(LD(5) * D))


def kernel_ld(desc, hp, x, xp=None, same=None, eps=EPS):
    mode = same_mode(xp, x, same)
    xq = x if mode != CROSS else xp
    K = None
    noise = None
    for t in split_hp(desc, hp, x.shape[0]):
        if t[0][0] == WN:
            noise = LD(t[0][1][0]) ** 2 if noise is None else noise
            continue
        T = None
        for kind, h in t:
            k = LD(h[0]) ** 2 * profile_ld(kind, factor_dist_ld(kind, h, x, xq))[0]
            T = k if T is None else T * k
        if mode != CROSS:
            T[np.diag_indices(T.shape[0])] += LD(eps)
        K = T if K is None else K + T
    assert K is not None, "kernel needs at least one stationary part"
    if mode == SELF and noise is not None:
        K[np.diag_indices(K.shape[0])] += noise
    return K


def find_factor(desc, i, d):
    """1-based i -> (term index, factor index in the term, 1-based index inside the factor)"""
    c = 0
    for ti, t in enumerate(terms(desc)):
        for fi, k in enumerate(t):
            if i <= c + width(k, d):
                return ti, fi, i - c
            c += width(k, d)
    raise IndexError(i)


class GradPieces:
    """What dK/dhp_i is made of, in long double: factor f (kind, h, loc = 1-based index inside the
    factor) of term t; Kf = sigma^2 f(D), W = -dKf/dD, D; the other factors of the term as
    (kind, h, D, value); and for loc > 1 the formula's prefactor pre, its geometry geo (r^2,
    (2 sin(pi r / p))^2 or r sin(2 pi r / p)) and q = r / p of a Periodic factor:
        loc = 1:  (2 / |sigma|) (Kf C + eps on the diagonal)
        loc > 1:  pre W C geo,     C = the product of the other factors' values"""


def grad_pieces(desc, i, hp, x):
    d = x.shape[0]
    ti, fi, loc = find_factor(desc, i, d)
    sp = split_hp(desc, hp, d)
    g = GradPieces()
    g.kind, g.h = sp[ti][fi]
    g.loc = loc
    if g.kind == WN:
        return g
    g.first = sum(len([k for k, _ in tt if k != WN]) for tt in sp[:ti])  # index into dist_bounds
    g.fi = fi
    g.s2 = LD(g.h[0]) ** 2
    g.D = factor_dist_ld(g.kind, g.h, x, x)
    f, w, g.P, _, _ = profile_ld(g.kind, g.D)
    g.Kf, g.W = g.s2 * f, g.s2 * w
    g.others = []
    for j, (kg, hg) in enumerate(sp[ti]):
        if j != fi:
            Dg = factor_dist_ld(kg, hg, x, x)
            g.others.append((j, kg, hg, Dg, LD(hg[0]) ** 2 * profile_ld(kg, Dg)[0]))
    g.C = functools.reduce(lambda a, b: a * b, [o[4] for o in g.others]) if g.others else None
    if loc == 1:
        g.pre = LD(2) / abs(LD(g.h[0]))
        return g
    k = (loc - 2) % d
    l = LD(g.h[1 + k])
    X = np.asarray(x, dtype=LD)
    g.r = X[k][:, None] - X[k][None, :]
    g.q = g.ch = None
    if g.kind != PER:
        g.geo, g.pre = g.r * g.r, LD(-2) * l
        return g
    p = LD(g.h[1 + d + k])
    g.q = g.r / p
    if loc <= d + 1:
        g.ch = LD(2) * np.sin(PI_LD * (g.q - np.rint(g.q)))
        g.geo, g.pre = g.ch * g.ch, LD(-2) * l
    else:
        sn = np.sin(PI_LD * LD(2) * (g.q - np.rint(g.q)))
        g.geo, g.pre = g.r * sn, LD(4) * PI_LD * l * l / (p * p)
    return g


def grad_value(g, n, eps):
    if g.kind == WN:
        return ("I", LD(2) * LD(g.h[0]))
    if g.loc == 1:
        T = g.Kf.copy() if g.C is None else g.Kf * g.C
        T[np.diag_indices(n)] += LD(eps)
        return g.pre * T
    return g.pre * (g.W if g.C is None else g.W * g.C) * g.geo


def kernel_grad_ld(desc, i, hp, x, eps=EPS):
    """dK/dhp_i (1-based); WhiteNoise -> ("I", 2 sigma_n)."""
    return grad_value(grad_pieces(desc, i, hp, x), x.shape[1], eps)


# ---------------------------------------------------------------------------------------
# features as the library forms them (fp64), their error bounds, the centre
# ---------------------------------------------------------------------------------------
def features(kind, h, x):
    """(s, e): the scaled or embedded points (de x n, float64: sincospi taken as correctly rounded)
    and the bound of each feature's error"""
    d = x.shape[0]
    l = np.asarray(h[1:d + 1], dtype=np.float64)[:, None]
    if kind != PER:
        s = x * l
        return s, U * np.abs(s)
    p = np.asarray(h[d + 1:], dtype=np.float64)[:, None]
    t = (2.0 * x) / p
    tr = (t - 2.0 * np.rint(t / 2.0)).astype(LD)  # exact
    cs = np.cos(PI_LD * tr).astype(np.float64)
    sn = np.sin(PI_LD * tr).astype(np.float64)
    e = np.abs(l) * (np.pi * U * np.abs(t) + 2.0 * U)
    return np.vstack([l * cs, l * sn]), np.vstack([e, e])


def centre(s):
    """(c, dc): the documented centre of the row points s and the bound of its own rounding"""
    cnt = min(s.shape[1], CENTER_PTS)
    c = np.sum(s[:, :cnt], axis=1) / float(cnt)
    return c, (cnt + 1) * U * np.max(np.abs(s[:, :cnt]), axis=1)


def dist_bounds(desc, hp, x, xp=None, same=None, form="gram"):
    """Per stationary factor (hp order) the worst-case rounding bound of D for every pair, as
    derived in the module docstring.  form: "gram" (B_gram) or "diff" (B_diff)."""
    assert form in ("gram", "diff")
    mode = same_mode(xp, x, same)
    out = []
    for t in split_hp(desc, hp, x.shape[0]):
        for kind, h in t:
            if kind == WN:
                continue
            sa, ea = features(kind, h, x)
            sb, eb = (sa, ea) if mode != CROSS else features(kind, h, xp)
            de = sa.shape[0]
            D = np.zeros((sa.shape[1], sb.shape[1]))
            A = np.zeros_like(D)
            for k in range(de):
                r = sa[k][:, None] - sb[k][None, :]
                D += r * r
                A += np.abs(r) * (ea[k][:, None] + eb[k][None, :])
            B = 2.0 * A + (de + 2) * U * D
            if form == "gram":
                c, dc = centre(sa)
                na = np.sum((np.abs(sa - c[:, None]) + dc[:, None]) ** 2, axis=0)
                nb = np.sum((np.abs(sb - c[:, None]) + dc[:, None]) ** 2, axis=0)
                B = B + (3 * de + 4) * U * (na[:, None] + nb[None, :])
            B *= _INFL
            if mode != CROSS:
                B[np.diag_indices(B.shape[0])] = 0.0  # the diagonal's D is 0 exactly
            out.append(B)
    return out


def centred_norms(kind, h, x):
    """|y_a|^2 of the row points of one factor about the documented centre (long double)"""
    s, _ = features(kind, h, x)
    c, _ = centre(s)
    y = s.astype(LD) - c.astype(LD)[:, None]
    return np.sum(y * y, axis=0)


def _w_ratio(kind, D, B):
    """w(max(D - B, 0)) / w(D) >= 1 of the profile's weight (float64, rounded up)"""
    if kind in (SE, PER):
        g = np.minimum(B, D.astype(np.float64) * _INFL)
    else:
        a = np.sqrt(LD(3 if kind == M32 else 5))
        g = (a * (np.sqrt(D) - np.sqrt(np.maximum(D - B.astype(LD), LD(0))))).astype(np.float64)
    # (Matern-5/2: w = (5/6) (1 + ar) e^-ar, whose factor 1 + ar only shrinks towards D - B)
    return np.exp(g) * _INFL


def _factor_value_and_bound(kind, h, D, Bs):
    """(k, [dk per B in Bs], W, zero, P): the factor's reference value, its element bound for each
    distance bound, W at the reference D, where the computed value must be exactly 0 (sigma^2
    exp(-arg) below half the least subnormal), and the profile's polynomial"""
    s2 = LD(h[0]) ** 2
    f, w, P, ar, dfdar = profile_ld(kind, D)
    k = s2 * f
    fixed = LD(E_TOT * U) * k + (P + LD(1)) * TINY
    if ar is not None:
        fixed = fixed + LD(U) * (LD(4) * k + LD(3) * ar * s2 * dfdar)
    dks = [(s2 * w * (_w_ratio(kind, D, B) * B).astype(LD) + fixed) * LD(_INFL) for B in Bs]
    expv = s2 * (f / P)
    zero = expv < (TINY / LD(2)) * LD(1.0 - 1e-9)
    return k, dks, s2 * w, zero, P


def element_bound(desc, hp, x, xp=None, same=None, eps=EPS, form="gram"):
    """(K_ref, bound, zero): |K - K_ref| <= bound elementwise for a kernel matrix built with the
    given distance form; zero marks the entries that must be exactly 0.0.  form may be a tuple of
    forms: bound is then the tuple of their bounds (the reference is evaluated once)."""
    forms = (form,) if isinstance(form, str) else tuple(form)
    mode = same_mode(xp, x, same)
    xq = x if mode != CROSS else xp
    Bs = [iter(dist_bounds(desc, hp, x, xp, same, f)) for f in forms]
    K = zero = None
    dK = [None] * len(forms)
    noise = None
    nterm = 0
    for t in split_hp(desc, hp, x.shape[0]):
        if t[0][0] == WN:
            noise = LD(t[0][1][0]) ** 2 if noise is None else noise
            continue
        vals = [_factor_value_and_bound(kind, h, factor_dist_ld(kind, h, x, xq), [next(b) for b in Bs])
                for kind, h in t]
        T = functools.reduce(lambda a, b: a * b, [v[0] for v in vals])
        for q in range(len(forms)):
            dT = np.zeros_like(T)
            for f in range(len(vals)):
                o = vals[f][1][q]
                for g in range(len(vals)):
                    if g != f:
                        o = o * (vals[g][0] + vals[g][1][q])
                dT += o
            dT += LD(len(vals) - 1) * (LD(U) * T + TINY)
            dK[q] = dT if dK[q] is None else dK[q] + dT
        z = functools.reduce(lambda a, b: a | b, [v[3] for v in vals])
        if mode != CROSS:
            T[np.diag_indices(T.shape[0])] += LD(eps)
            z[np.diag_indices(T.shape[0])] = False
        K = T if K is None else K + T
        zero = z if zero is None else zero & z
        nterm += 1
    if mode == SELF and noise is not None:
        K[np.diag_indices(K.shape[0])] += noise
    nadd = np.full(K.shape, float(nterm - 1))
    if mode != CROSS:
        nadd[np.diag_indices(K.shape[0])] += nterm + (1 if mode == SELF and noise is not None else 0)
    adds = LD(U * _INFL) * nadd.astype(LD) * np.abs(K)
    out = tuple(b + adds for b in dK)
    return K, out[0] if isinstance(form, str) else out, zero


# ---------------------------------------------------------------------------------------
# the bound of dK/dhp_i (gpr_kernel_grad's kgrad_kernel, the fused MLL gradient of mll.hip)
# ---------------------------------------------------------------------------------------
# Both form D in the difference form (B_diff) and each factor's value and W from it.  Rounding
# counts, in units of u relative to the quantity named, beside the kernel lines they come from
# (assembly.hip, kgrad_kernel; the fused pass forms the same products per pair and sums them):
#
#   kprof_exact_w(prof, sig * sig, s, &W)   value: E_TOT, as in the K build (library exp 2 + sigma^2
#                                           2, or the table's 4.5)
#                                           W = 1.5 e | (5/6) (e poly): E_TOT + 4 (a r: 3, product: 1)
#                                           W moves with D by -dW/dD B_diff, -dW/dD at max(D - B, 0)
#       s2 * exp(-D), e * poly              sigma^2 enters AFTER the exponential was rounded into
#                                           the subnormals: (sigma^2 + 1) P 2^-1074 absolute
#   Kp *= C;  W *= C                        1 and 2^-1074 per cofactor product
#   (2.0 / fabs(sig)) * Kp  [+ eps]         GRAD_U_SIGMA = 4: quotient, product, eps, slack 1
#   dx = X[a] - X[b]; dx * dx               the difference u (2u in the square), the square u
#   -2.0 * l * W * (dx * dx)                three products                     GRAD_U_FORMULA = 8
#   2.0 * sinpi(dx / pk); ch * ch           angle of sinpi(fl(fl(dx) / p)): 2 pi u |r / p|, sinpi u;
#                                           d(ch^2) = 2 |ch| 2 (2 pi u |q| + u)
#   (4 pi l l / (pk pk)) W dx sinpi(2 dx / pk)   angle 4 pi u |r / p|, sinpi u: |r| (4 pi u |q| + u);
#                                           the prefactor's and the products' roundings in the 8
#   every product landing in the subnormals rounds by half a step more, scaled by the factors
#   still to come: (|geo| + 2) 2^-1074 for the formula's last products, 2^-1074 for loc = 1
GRAD_U_SIGMA = 4.0
GRAD_U_FORMULA = 8.0
GRAD_U_W = E_TOT + 4.0


def _late_sigma(s2, P):
    return (s2 + LD(1)) * TINY * P


def _cofactor_bound(g, Bs):
    """(C, dC): the product of the other factors' values and its bound"""
    C = dC = None
    for j, kg, hg, Dg, vg in g.others:
        _, dg, _, _, Pg = _factor_value_and_bound(kg, hg, Dg, [Bs[g.first + j]])
        dg = dg[0] + _late_sigma(LD(hg[0]) ** 2, Pg)
        dC = dg if C is None else dC * (vg + dg) + C * dg + LD(U) * C * vg + TINY
        C = vg if C is None else C * vg
    return C, dC


def _times_cofactor(v, dv, C, dC):
    """bound of fl(v C) given those of v and C"""
    return dv if C is None else dv * (C + dC) + v * dC + LD(U) * v * C + TINY


def grad_bound(g, v, Bs):
    """The element bound of dK/dhp_i for the pieces g, its value v and the per-factor B_diff."""
    if g.kind == WN:
        return LD(2 * U) * abs(LD(g.h[0]))
    B = Bs[g.first + g.fi]
    C, dC = _cofactor_bound(g, Bs)
    if g.loc == 1:
        dKf = _factor_value_and_bound(g.kind, g.h, g.D, [B])[1][0] + _late_sigma(g.s2, g.P)
        dT = _times_cofactor(g.Kf, dKf, C, dC)
        return (g.pre * dT + LD(GRAD_U_SIGMA * U) * np.abs(v) + TINY) * LD(_INFL)
    Bl = B.astype(LD)
    dW = g.s2 * neg_dw_ld(g.kind, np.maximum(g.D - Bl, LD(0))) * Bl + LD(GRAD_U_W * U) * g.W \
        + _late_sigma(g.s2, g.P)
    dWC = _times_cofactor(g.W, dW, C, dC)
    WC = g.W if C is None else g.W * C
    if g.q is None:
        dgeo = LD(0)
    elif g.ch is not None:        # a Periodic length-scale: geo = ch^2
        dgeo = LD(2) * np.abs(g.ch) * LD(2) * (LD(2) * PI_LD * LD(U) * np.abs(g.q) + LD(U))
    else:                         # a period: geo = r sin(2 pi q)
        dgeo = np.abs(g.r) * (LD(4) * PI_LD * LD(U) * np.abs(g.q) + LD(U))
    bound = abs(g.pre) * (dWC * (np.abs(g.geo) + dgeo) + WC * dgeo) \
        + LD(GRAD_U_FORMULA * U) * np.abs(v) + (np.abs(g.geo) + LD(2)) * TINY
    return bound * LD(_INFL)


def kernel_grad_bound(desc, i, hp, x, eps=EPS):
    """(dK_i, bound); WhiteNoise: (("I", lam), the bound of lam)"""
    g = grad_pieces(desc, i, hp, x)
    v = grad_value(g, x.shape[1], eps)
    Bs = None if g.kind == WN else dist_bounds(desc, hp, x, None, SELF, "diff")
    return v, grad_bound(g, v, Bs)


# ---------------------------------------------------------------------------------------
# fp64 emulation of the two distance forms and of the table exponential (CPU tests)
# ---------------------------------------------------------------------------------------
def emulate_dist(kind, h, x, xp=None, form="gram", xp_own_centre=False):
    """D^ as the kernels form it, in float64 NumPy (products rounded on their own).  xp_own_centre
    is the mutation the CPU tests use to show that a family notices a centre per operand."""
    sa, _ = features(kind, h, x)
    sb = sa if xp is None else features(kind, h, xp)[0]
    de = sa.shape[0]
    D = np.zeros((sa.shape[1], sb.shape[1]))
    if form == "diff":
        for k in range(de):
            r = sa[k][:, None] - sb[k][None, :]
            D = D + r * r
        return D
    c, _ = centre(sa)
    cb = centre(sb)[0] if xp_own_centre else c
    ya, yb = sa - c[:, None], sb - cb[:, None]
    na, nb = np.zeros(ya.shape[1]), np.zeros(yb.shape[1])
    for k in range(de):
        na = na + ya[k] * ya[k]
        nb = nb + yb[k] * yb[k]
    acc = (-na)[:, None] + (-nb)[None, :]
    for k in range(de):
        acc = acc + (2.0 * ya[k])[:, None] * yb[k][None, :]
    D = -acc
    if xp is None:
        D[np.diag_indices(D.shape[0])] = 0.0
    return D


@functools.lru_cache(maxsize=None)
def _exp_table():
    j = np.arange(256, dtype=LD)
    return np.exp(j * LN2_LD / LD(256)).astype(np.float64)


def emulate_kexp(dist, sigma, clamp=True):
    """kexp_s2 of kexp.hpp step by step in float64 NumPy (clamp=False: kexp_s2_nc, the int32
    wrap of n included); the multiply-adds are not fused."""
    dist = np.asarray(dist, dtype=np.float64)
    x = np.where(dist > 800.0, -800.0, -dist) if clamp else -dist
    magic = 6755399441055744.0
    kf = x * 369.3299304675746 + magic
    nf = kf - magic
    r = nf * -0.00270760617331689 + x
    r = nf * -7.453964567463233e-13 + r
    ni = (kf.view(np.int64) & 0xffffffff).astype(np.uint32).view(np.int32).astype(np.int64)
    p = r * 0.041666666666666664 + 0.16666666666666666
    p = r * p + 0.5
    p = r * p
    q = r * p + r
    t = ((sigma * sigma) * _exp_table())[ni & 255]
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(t * q + t, (ni >> 8).astype(np.int64))


# ---------------------------------------------------------------------------------------
# input families: (x, xp, hp), preconditions asserted in long double
# ---------------------------------------------------------------------------------------
def family_hp(desc, d, l0, sigma=1.0, period=None):
    """sigma for the first stationary factor and 0.8 sigma for the others; l0 (d values) for the
    first, 0.7 l0 (1 + 0.05 k) for the others; Periodic p_k = period_k; noise 0.1 sigma."""
    l0 = np.broadcast_to(np.asarray(l0, dtype=np.float64), (d,))
    hp, p = [], 0
    for k in flat(desc):
        if k == WN:
            hp += [0.1 * sigma]
            continue
        hp += [sigma if p == 0 else 0.8 * sigma]
        hp += list(l0 if p == 0 else 0.7 * l0 * (1.0 + 0.05 * np.arange(d)))
        if k == PER:
            hp += list(np.broadcast_to(np.asarray(period, dtype=np.float64), (d,)))
        p += 1
    return np.array(hp)


def assert_north_star(desc, hp, x, xp, skip=()):
    """The bounds scale with |y|^2, so a family must keep them meaningful: B_gram <= 1e-8 (the
    project's north-star tolerance) for every pair with D_ref < 40, symmetric and cross, outside
    the rows and columns listed in skip.  Returns the largest such B."""
    worst = 0.0
    for xq in (None, xp):
        Bs = dist_bounds(desc, hp, x, xq, None, "gram")
        fs = [kh for t in split_hp(desc, hp, x.shape[0]) for kh in t if kh[0] != WN]
        for (kind, h), B in zip(fs, Bs):
            D = factor_dist_ld(kind, h, x, x if xq is None else xq)
            near = np.asarray(D < 40)
            if len(skip):
                near[list(skip), :] = False
                if xq is None:
                    near[:, list(skip)] = False
            if near.any():
                worst = max(worst, float(B[near].max()))
    assert worst <= NORTH_STAR, f"B_gram reaches {worst:.3g} on pairs with D < 40"
    return worst


F1_TIES = (1, 255, 256, 1000, 65535, 131072, 200000)
F1_BANDS = (36.0, 100.0, 700.0,
            708.3, 708.35, 708.39, 708.4, 708.45, 708.5,          # normal / subnormal edge
            740.0, 742.0, 744.0, 744.4, 744.5, 745.0, 745.1,      # the last non-zero values
            745.2, 750.0, 799.9, 800.1,                           # exactly 0
            1e4, 1e7)


def f1_targets():
    """(target D, lo, hi) of every rung: the realised D must lie in (lo, hi)"""
    out = [(1e-20, 0.99e-20, 1.01e-20), (1e-8, 0.99e-8, 1.01e-8)]
    step = LN2_LD / LD(256)
    for j in F1_TIES:
        for c in (LD(j) * step, (LD(j) + LD(0.5)) * step):  # r changes sign / n changes (a tie)
            out.append((c - LD(5e-13), c - LD(1e-12), c))
            out.append((c + LD(5e-13), c, c + LD(1e-12)))
    for b in F1_BANDS:
        w = max(1e-9 * b, 1e-9)
        out.append((b, b - w, b + w))
    return out


def f1_ladder(desc, sigma=1.0):
    """The exp ladder: d = 3, n = 192, m = 80.  x[:, 0] is the base (0, .5, .5), x[:, 1] its copy,
    then one rung per target at (sqrt(D), .5, .5) with l = 1 exactly for the first factor, so that
    the realised D between the base and a rung is the rung's square; the rest in the unit cube.
    xp: the base, every fourth rung, and cube points."""
    d, n, m = 3, 192, 80
    rng = np.random.default_rng(101)
    x, xp = rng.random((d, n)), rng.random((d, m))
    tg = f1_targets()
    pos = np.array([float(np.sqrt(LD(t[0]))) for t in tg])
    assert 2 + len(tg) <= n
    x[:, 0] = x[:, 1] = (0.0, 0.5, 0.5)
    x[0, 2:2 + len(tg)] = pos
    x[1:, 2:2 + len(tg)] = 0.5
    xp[:, 0] = (0.0, 0.5, 0.5)
    sub = pos[::4]
    xp[0, 1:1 + len(sub)] = sub
    xp[1:, 1:1 + len(sub)] = 0.5
    hp = family_hp(desc, d, 1.0, sigma, period=(0.9, 1.0, 1.1))
    # preconditions
    first = split_hp(desc, hp, d)[0][0] if terms(desc)[0] != [WN] else None
    assert first is not None and np.all(first[1][1:d + 1] == 1.0)
    real = LD(x[0, 2:2 + len(tg)]) ** 2
    for (t, lo, hi), r in zip(tg, real):
        assert LD(lo) < r < LD(hi), (t, r)
    if first[0] != PER:
        Dk = factor_dist_ld(first[0], first[1], x, x)
        assert Dk[0, 1] == 0 and np.all(Dk[0, 2:2 + len(tg)] == real)
        assert np.all(factor_dist_ld(first[0], first[1], x, xp)[2:2 + len(tg), 0] == real)
    return x, xp, hp


def f2_far(desc, c0, d, n=130, m=97):
    """Far from the origin: x = c0 + cube, l_k = 0.75 sqrt(8/d) within 5 %."""
    rng = np.random.default_rng(int(c0) % 1000 + d + n)
    x, xp = c0 + rng.random((d, n)), c0 + rng.random((d, m))
    hp = family_hp(desc, d, 0.75 * np.sqrt(8.0 / d) * rng.uniform(0.95, 1.05, d), period=1.0)
    assert np.all(x >= c0) and np.all(xp >= c0)
    return x, xp, hp


def f3a_grid(desc):
    """d = 1, a sorted grid of n = 2304 > 2048 points, neighbour D = 0.1 (l = 1), the m = 130 cross
    points beside the far end: the centre (the first 2048 points' mean) is 280 spacings away from
    the middle of the data and 1215 from the cross points."""
    n, m = 2304, 130
    h = float(np.sqrt(LD(0.1)))
    x = (np.arange(n) * h)[None, :]
    xp = x[:, n - m:] + 0.37 * h
    hp = family_hp(desc, 1, 1.0, period=1.0)
    assert n > CENTER_PTS and np.all(np.diff(x[0]) > 0)
    Dn = (LD(x[0, 1:]) - LD(x[0, :-1])) ** 2
    assert np.all(np.abs(Dn - LD(0.1)) < 1e-12)
    return x, xp, hp


F3B_SPREAD = 2300.0


def f3b_spread(desc):
    """d = 8, n = 600, axis 0 sorted and spanning F3B_SPREAD length-scales (uniform draws, so that
    neighbours are close), the other axes in the unit cube.  2300 is the widest spread the 1e-8
    cap allows with the derived coefficient 3d + 4 (4000 length-scales: 28 u 2 (2000)^2 =
    2.5e-8)."""
    d, n, m = 8, 600, 97
    rng = np.random.default_rng(38)
    l = 0.75 * rng.uniform(0.95, 1.05, d)
    x, xp = rng.random((d, n)), rng.random((d, m))
    x[0] = np.sort(rng.random(n)) * F3B_SPREAD / l[0]
    x[0, 0], x[0, -1] = 0.0, F3B_SPREAD / l[0]
    xp[0] = rng.random(m) * F3B_SPREAD / l[0]
    hp = family_hp(desc, d, l, period=1.0)
    assert np.all(np.diff(x[0]) >= 0) and abs(LD(x[0, -1]) * LD(l[0]) - LD(F3B_SPREAD)) < 1e-9
    return x, xp, hp


F4_IDX = (5, 300, 500, 700, 1039)
F4_NEAR = (5, 300, 700, 1039)  # the points just below the limit
KU_NC_LIM = 1.4e6
KU_W, KU_H, KU_SEG = 32, 32, 128  # assembly.hip: strip width, unit height, rows per work item


def kup_unit_class(row, col, n, full):
    """Which unit of kmat_symu_kernel computes element (row, col), by assembly.hip's index
    arithmetic: "diag" and "edge" units always take the clamped exponential, "interior" ones only
    if some |y|^2 of theirs reaches KU_NC_LIM; None if the build does not write the element.
    full: gpr_kernel's build of every row; else the fit's, rows [0, 128 (col / 128 + 1))."""
    j0, r0, i0 = KU_W * (col // KU_W), KU_SEG * (row // KU_SEG), KU_H * (row // KU_H)
    rows = n if full else min(n, 128 * (j0 // 128 + 1))
    r1 = min(r0 + KU_SEG, rows)
    if row >= r1:
        return None
    if i0 <= j0 < i0 + KU_H:
        return "diag"
    return "edge" if j0 + KU_W > n or i0 + KU_H > r1 else "interior"


def kup_item_is_column_store(row, col, n):
    """Whether the fit's single-part build takes (row, col) through kup_item_cols"""
    j0, r0 = KU_W * (col // KU_W), KU_SEG * (row // KU_SEG)
    r1 = min(r0 + KU_SEG, min(n, 128 * (j0 // 128 + 1)))
    return r1 - r0 == KU_SEG and j0 + KU_W <= n and not (r0 <= j0 < r1)


def f4_planted(desc, d, variant):
    """Around KU_NC_LIM, for the fit's upper-only build: n = 1040, cube data, and planted points
    along axis 0 at first-factor length-scales from the centre:
      5 (a diagonal unit) at -1150, 300 at +1161.9, 700 at -1161.9 (both interior to their
      strips and 128-row segments), 1039 (the ragged last strip and unit) at +1150: every
      |y|^2 in [1.30e6, 1.39e6], just below the limit, and opposite-side pairs at D ~ 5.4e6, the
      top of kexp_s2_nc's proven range (n = 2.0e9 of the int32's 2.147e9).  Element (300, 700) --
      and (5, 300) -- lies in a unit that is neither diagonal nor an edge, in the fit's build (a
      column-store item when there is one part) and in gpr_kernel's full build, both triangles:
      asserted below from the kernel's index arithmetic.  (5, 1039) and (700, 1039) meet the
      same distances in the clamped edge units.
      "i":  500 at +100 (|y|^2 ~ 1e4).  No unit needs the clamp.
      "ii": 500 at +5100: |y|^2 >= 2.5e7 -- every strip, unit and item it touches must clamp (an
            unclamped D ~ 4e7 wraps n past int32); it moves the centre by 4.9, which keeps the
            other four inside their range.
    Returns (x, None, hp); asserts, with the centre and |y|^2 as the library documents them, on
    which side of 1.4e6 each planted point falls for the first factor, and that every other point
    and every other factor stays below."""
    assert variant in ("i", "ii")
    n = 1040
    rng = np.random.default_rng(7 * d + len(variant))
    l = 0.75 * np.sqrt(8.0 / d) * rng.uniform(0.95, 1.05, d)
    x = rng.random((d, n))
    x[0, 5], x[0, 1039] = 0.5 - 1150.0 / l[0], 0.5 + 1150.0 / l[0]
    x[0, 300], x[0, 700] = 0.5 + 1161.9 / l[0], 0.5 - 1161.9 / l[0]
    x[0, 500] = 0.5 + (5100.0 if variant == "ii" else 100.0) / l[0]
    hp = family_hp(desc, d, l)
    fs = [kh for t in split_hp(desc, hp, d) for kh in t if kh[0] != WN]
    q = centred_norms(*fs[0], x)
    for a in F4_NEAR:
        assert 1.30e6 <= q[a] <= 1.39e6, (a, q[a])
    s0 = features(*fs[0], x)[0][0]
    c0 = centre(features(*fs[0], x)[0])[0][0]
    for a, b in ((300, 700), (5, 300), (5, 1039), (700, 1039)):  # opposite sides, D at the top
        assert (s0[a] - c0) * (s0[b] - c0) < 0
        D = factor_dist_ld(*fs[0], x[:, [a]], x[:, [b]])[0, 0]
        assert 5.25e6 < D < 5.6e6 and 2 * (q[a] + q[b]) < 5.6e6, (a, b, D)
    for a, b in ((300, 700), (5, 300)):
        assert kup_unit_class(a, b, n, False) == "interior" and kup_item_is_column_store(a, b, n)
        assert kup_unit_class(a, b, n, True) == "interior" and kup_unit_class(b, a, n, True) == "interior"
    assert kup_unit_class(5, 5, n, False) == "diag" and kup_unit_class(5, 1039, n, False) == "edge"
    assert kup_unit_class(1039, 1039, n, True) in ("diag", "edge")
    assert kup_unit_class(300, 500, n, False) == "interior" and kup_unit_class(500, 700, n, False) == "interior"
    if variant == "ii":
        assert q[500] >= 2.5e7, q[500]
    else:
        assert q[500] < 2e4
    rest = np.ones(n, dtype=bool)
    rest[list(F4_IDX)] = False
    assert q[rest].max() < 100.0
    for kh in fs[1:]:
        qq = centred_norms(*kh, x)
        assert qq[rest].max() < 100.0 and all(qq[a] < KU_NC_LIM for a in F4_NEAR)
    return x, None, hp


def f5_periodic(desc):
    """d = 2, n = 130, m = 97: x up to 1e4 with p ~ 1 (|x/p| up to 1e4 periods); a SquaredExp factor
    beside the Periodic one gets l = 1e-4, so that the product is not all zeros."""
    d, n, m = 2, 130, 97
    rng = np.random.default_rng(55)
    x, xp = rng.random((d, n)) * 1e4, rng.random((d, m)) * 1e4
    x[:, 0], x[:, 1] = (1e4, 1e4), (0.0, 1e4)
    hp, p = [], 0
    for k in flat(desc):
        if k == WN:
            hp += [0.1]
        elif k == PER:
            hp += [1.0 if p == 0 else 0.8] + [0.8, 0.6] + [0.93, 1.07]
            p += 1
        else:
            hp += [1.0 if p == 0 else 0.8] + [1.0e-4, 0.7e-4]
            p += 1
    assert PER in flat(desc) and x.max() == 1e4
    return x, xp, np.array(hp)
