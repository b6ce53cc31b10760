"""GPU: the matrix-free gradient form g_j = sum_ab (A B')_ab dK_ab/dhp_j (gpr_kernel_grad_form)
against the long-double dK of kernel_ref_ld.py summed in long double.

Inputs in the unit cube, hyper-parameters in [0.3, 2] (the range of the project's 1e-13 bar for
kernel entries), A and B standard normal.  Componentwise bound, u = 2^-53:
    |g_j - ref_j| <= (1e-13 + (n + r + 2d + 16) u) T_j
-- 1e-13 for K_p and W_p, r u for the weight tile, 2d u for the second product and the per-point
dots, n + 16 for any summation order and the remaining products -- with T_j the sum of the absolute
values of every term the kernel adds for slot j, |A| |B|' in M's place, times the factor the host
applies to the slot (T_j is in g_j's units):
    sigma:    (2 / |sigma|) sum |M| (K_p + eps on the diagonal)
    l_k:      (2 / l_k) sum |M| W_p (y_ak^2 + y_bk^2 + 2 |y_ak y_bk|),  y the centred scaled points
    sigma_n:  2 sigma_n sum_a |M|_aa
"""
import ctypes

import numpy as np
import pytest
import torch

import kernel_ref_ld as R
import test_product_cpu as PR
from kernel_ref_ld import LD, M32, M52, PER, SE, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

DESCS = {"SE": [SE], "M32": [M32], "SE+M52+WN": [SE, M52, WN], "5SE+WN": [SE, SE, SE, SE, SE, WN]}

# (description, d, n, r, GPR_KGF_SLABS, lda - n = ldb - n)
CASES = [
    ("SE", 1, 1, 1, 0, 0),
    ("SE", 8, 64, 4, 0, 0),             # one full tile: the operand layouts
    ("SE", 8, 63, 17, 0, 0),            # a ragged k-step of r
    ("SE", 8, 65, 1, 1, 0),
    ("SE", 8, 200, 70, 3, 0),           # r beyond the register-held block, ragged last slab
    ("SE", 21, 129, 17, 0, 0),          # run-time S, 42 columns of V
    ("SE", 40, 200, 4, 3, 0),           # 80 columns: two passes
    ("M32", 1, 129, 4, 1, 0),
    ("M32", 8, 64, 17, 0, 0),
    ("M32", 21, 65, 70, 0, 0),
    ("M32", 40, 63, 1, 0, 0),
    ("SE+M52+WN", 8, 1, 1, 0, 0),
    ("SE+M52+WN", 1, 64, 70, 0, 0),
    ("SE+M52+WN", 8, 200, 17, 3, 0),
    ("SE+M52+WN", 12, 129, 17, 3, 0),   # 24 columns of V: two parts per launch, two launches
    ("SE+M52+WN", 21, 200, 4, 0, 0),
    ("SE+M52+WN", 40, 129, 17, 1, 0),
    ("5SE+WN", 1, 200, 1, 0, 0),
    ("5SE+WN", 8, 129, 4, 3, 0),        # two part groups, the noise with the last
    ("5SE+WN", 21, 63, 17, 0, 0),
    ("5SE+WN", 40, 65, 4, 0, 0),
    ("SE+M52+WN", 8, 65, 17, 0, 7),     # NaN rows between the factors' columns
    ("SE+M52+WN", 3, 1100, 4, 0, 0),    # n > 1024: the trace's second stage, the default slabs
    ("SE", 3, 1100, 17, 3, 0),
]


def form_ref(desc, hp, x, M, Mabs, eps=R.EPS):
    """(ref, T, S): ref_j = sum M o dK_j, T_j as in the module docstring with Mabs in M's place,
    S_j = sum Mabs o |dK_j| -- long double, for every hyper-parameter j"""
    d, n = x.shape
    ref, T, S = [], [], []
    dg = np.trace(M), np.trace(Mabs)
    for j in range(1, len(hp) + 1):
        g = R.grad_pieces(desc, j, hp, x)
        if g.kind == WN:
            lam = LD(2) * LD(g.h[0])
            ref.append(lam * dg[0]), T.append(abs(lam) * dg[1]), S.append(abs(lam) * dg[1])
            continue
        dK = R.grad_value(g, n, eps)
        ref.append(np.sum(M * dK)), S.append(np.sum(Mabs * np.abs(dK)))
        if g.loc == 1:
            T.append(S[-1])
            continue
        s, _ = R.features(g.kind, g.h, x)
        k = g.loc - 2
        y = np.abs(s[k].astype(LD) - LD(R.centre(s)[0][k]))
        T.append(np.sum(Mabs * g.W * (y[:, None] + y[None, :]) ** 2) * LD(2) / abs(LD(g.h[1 + k])))
    return np.array(ref), np.array(T), np.array(S)


def _inputs(name, d, n, r, seed):
    rng = np.random.default_rng(seed)
    desc = DESCS[name]
    hp = rng.uniform(0.3, 2.0, sum(R.width(k, d) for k in R.flat(desc)))
    return desc, hp, rng.random((d, n)), rng.standard_normal((n, r)), rng.standard_normal((n, r))


def _run(desc, hp, x, A, B, pad=0, log_scale=False):
    """through gpr_amd.kernel_grad_form, the factors as device buffers whose padding rows are NaN"""
    ctx = G.default_context()
    n, r = A.shape
    dev = []
    for F in (A, B):
        t = torch.full((r, n + pad), float("nan"), dtype=torch.float64, device=ctx.device)
        t[:, :n] = torch.from_numpy(np.ascontiguousarray(F.T)).to(ctx.device)
        dev.append(t)
    torch.cuda.synchronize()
    return G.kernel_grad_form(PR.cov_of(desc), hp, x, dev[0], dev[1], log_scale=log_scale)


@pytest.mark.parametrize("name,d,n,r,slabs,pad", CASES)
def test_form_against_long_double(knobs, name, d, n, r, slabs, pad):
    knobs("GPR_KGF_SLABS", slabs)
    desc, hp, x, A, B = _inputs(name, d, n, r, 1000 * n + 10 * r + d)
    g = _run(desc, hp, x, A, B, pad)
    Al, Bl = A.astype(LD), B.astype(LD)
    ref, T, _ = form_ref(desc, hp, x, Al @ Bl.T, np.abs(Al) @ np.abs(Bl).T)
    bound = (1e-13 + (n + r + 2 * d + 16) * R.U) * T
    err = np.abs(g.astype(LD) - ref)
    print(f"max |err| / bound = {float(np.max(err / np.where(bound > 0, bound, 1))):.3g}")
    assert np.all(np.isfinite(g))
    assert np.all(err <= bound)


def test_two_calls_agree_bit_for_bit(knobs):
    knobs("GPR_KGF_SLABS", 3)
    desc, hp, x, A, B = _inputs("SE+M52+WN", 8, 200, 17, 5)
    assert np.array_equal(_run(desc, hp, x, A, B), _run(desc, hp, x, A, B))


@pytest.mark.parametrize("name,d,n,r", [("SE+M52+WN", 1, 64, 70), ("SE", 8, 63, 17),
                                        ("5SE+WN", 21, 63, 17)], ids=["S=1", "S=2", "run-time S"])
def test_log_scale_is_one_multiplication_by_hp(name, d, n, r):
    """log_scale: grad .*= hp on the host after the form, so the result is the plain call's (two
    calls agree bit for bit) times hp[i], rounded once"""
    desc, hp, x, A, B = _inputs(name, d, n, r, 1000 * n + 10 * r + d)
    g = _run(desc, hp, x, A, B)
    gl = _run(desc, hp, x, A, B, log_scale=True)
    assert np.all(np.isfinite(g)) and np.all(g != 0.0)
    assert np.array_equal(gl, g * hp)


# (what changes, the word the message must carry)
BAD_ARGS = [(dict(dX=None), "dX is"), (dict(dA=None), "dA is"), (dict(dB=None), "dB is"),
            (dict(grad=None), "grad is"), (dict(n=0), "n="), (dict(r=0), "r="),
            (dict(lda=-1), "lda"), (dict(ldb=-1), "ldb")]


@pytest.mark.parametrize("change,word", BAD_ARGS, ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in BAD_ARGS])
def test_argument_errors(change, word):
    """GPR_E_ARG naming the argument, before anything is written"""
    from gpr_amd import _lib as L, core
    ctx = G.default_context()
    desc, hp, x, A, B = _inputs("SE+M52+WN", 3, 70, 4, 9)
    d, n = x.shape
    kinds, nk = core._kinds_arr(PR.cov_of(desc))
    g = np.full(len(hp), -7.5)
    a = dict(dX=ctx.colmajor(x), n=n, dA=ctx.colmajor(A), lda=n, dB=ctx.colmajor(B), ldb=n, r=4,
             grad=g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    a.update(change)
    for k in ("lda", "ldb"):  # -1: one short of n
        a[k] = n - 1 if a[k] == -1 else a[k]
    rc = L.lib.gpr_kernel_grad_form(ctx.h, kinds, nk, core._hp_arr(hp)[1], d, core._ptr(a["dX"]),
                                    a["n"], core._ptr(a["dA"]), a["lda"], core._ptr(a["dB"]),
                                    a["ldb"], a["r"], R.EPS, 0, a["grad"])
    msg = L.lib.gpr_last_error(ctx.h).decode()
    assert rc == -1, (rc, msg)  # GPR_E_ARG
    assert word in msg, msg
    assert np.all(g == -7.5)


@pytest.mark.parametrize("desc", [[PER], [[SE, PER], WN]], ids=["PER", "SE*PER+WN"])
def test_periodic_and_product_are_refused(desc):
    from gpr_amd import _lib as L, core
    ctx = G.default_context()
    d, n, r = 3, 70, 4
    rng = np.random.default_rng(9)
    hp = rng.uniform(0.3, 2.0, sum(R.width(k, d) for k in R.flat(desc)))
    kinds, nk = core._kinds_arr(PR.cov_of(desc))
    dx, dA = ctx.colmajor(rng.random((d, n))), ctx.colmajor(rng.standard_normal((n, r)))
    g = np.full(len(hp), -7.5)
    rc = L.lib.gpr_kernel_grad_form(ctx.h, kinds, nk, core._hp_arr(hp)[1], d, core._ptr(dx), n,
                                    core._ptr(dA), n, core._ptr(dA), n, r, R.EPS, 0,
                                    g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == -4  # GPR_E_UNSUP
    assert np.all(g == -7.5)
