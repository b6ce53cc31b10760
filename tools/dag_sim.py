"""Discrete-event model of the persistent tile-DAG launch (csrc/dag.hip) to study task orders
on the CPU.  Not a test and not the product path.

Model: W workgroups take tasks in ticket order (greedy list scheduling: the next ticket goes
to the first workgroup that frees up).  A task of tile (i, j) (or right-hand-side tile (i, c))
loads its tile (c_load), accumulates row blocks k < i in order, block k not before both
inputs (tile (k, i) of A and tile (k, j) of A or B) are final (c_step per block), then
  diagonal:      factors the tile and writes W_i (c_fac)                   -> final
  off-diagonal:  waits for W_i (the diagonal task of row i), U_ij = W_i^T B (c_tri) -> final
Final tiles become visible to waiters c_pub later.  Times in microseconds.

    python tools/dag_sim.py                 (calibration against the measured launches)
"""
import argparse
import heapq

import numpy as np


def task_list(nt, ntr, rlag=0, fearly=False, lower=False, zlag=2, order="rows", group=2, skew=0,
              gmin=0):
    """The host-built ticket order of launch_potrf_dag (dag.hip), or an alternative.
    order="groups": dag.hip's dag_task_order for plain launches -- rows below gmin (rounded up
    to a multiple of group) in row order, then `group` rows at a time, a group's tasks merged by
    column with member r `r * skew` column slots behind member 0 (A's tiles, then the
    right-hand-side tiles)."""
    tasks = []
    lag = min(zlag if lower else rlag, nt)

    def rhs_row(i):
        for c in range(min(ntr, i + 1) if lower else ntr):
            tasks.append(("R", i, c))

    if order == "groups":
        assert not lower and not fearly and rlag == 0
        g0 = min(nt, (gmin + group - 1) // group * group)
        sk = min(skew, max(nt, ntr))
        for i in range(g0):
            tasks.extend(("A", i, j) for j in range(i, nt))
            rhs_row(i)
        for g in range(g0, nt, group):
            m = min(group, nt - g)
            for s in range(nt - g + (m - 1) * sk):
                for r in range(m):
                    j = g + s - r * sk
                    if g + r <= j < nt:
                        tasks.append(("A", g + r, j))
            for s in range(ntr + (m - 1) * sk):
                for r in range(m):
                    if 0 <= s - r * sk < ntr:
                        tasks.append(("R", g + r, s - r * sk))
    elif order == "rows":
        for i in range(nt):
            if not fearly or i == 0:
                tasks.append(("A", i, i))
            for j in range(i + 1, nt):
                tasks.append(("A", i, j))
                if fearly and j == i + 1:
                    tasks.append(("A", j, j))
            if i - lag >= 0:
                rhs_row(i - lag)
        for i in range(max(nt - lag, 0), nt):
            rhs_row(i)
    elif order.startswith("cols"):
        # right-looking-friendly: tile (i, j) in column-major order of j, then RHS by rows
        for j in range(nt):
            for i in range(j + 1):
                tasks.append(("A", i, j))
            if j - lag >= 0:
                rhs_row(j - lag)
        for i in range(max(nt - lag, 0), nt):
            rhs_row(i)
    return tasks


def simulate(nt, ntr, tasks, W=256, c_step=14.8, c_load=1.5, c_fac=48.0, c_tri=7.4, c_pub=1.5,
             lower=False, rhs_step=None, kstep=None, starts=None):
    """starts: a dict to fill with every task's start time (the partners' start gaps)."""
    rhs_step = c_step if rhs_step is None else rhs_step
    finA = np.full((nt, nt), np.inf)
    finR = np.full((nt, max(ntr, 1)), np.inf)
    if lower:  # identity's zero tiles above the diagonal: final from the start
        for c in range(ntr):
            finR[:c, c] = 0.0
    free = [0.0] * W
    heapq.heapify(free)
    busy = 0.0
    end = 0.0
    for kind, i, j in tasks:
        t0 = heapq.heappop(free)
        if starts is not None:
            starts[(kind, i, j)] = t0
        t = t0 + c_load
        k0 = j if (kind == "R" and lower) else 0
        step = c_step if kind == "A" else rhs_step
        if i > k0:
            a = np.maximum(finA[k0:i, i], finA[k0:i, j] if kind == "A" else finR[k0:i, j]) + c_pub
            K = i - k0
            t = max(t + K * step, float(np.max(a + step * np.arange(K, 0, -1))))
        if kind == "A" and i == j:
            t += c_fac
            finA[i, i] = t
        else:
            t = max(t, finA[i, i] + c_pub) + c_tri
            if kind == "A":
                finA[i, j] = t
            else:
                finR[i, j] = t
        busy += t - t0
        end = max(end, t)
        heapq.heappush(free, t)
    return end, busy / (W * end)


def flops(nt, ntr, lower=False):
    n = nt * 128.0
    f = n ** 3 / 3
    f += (n ** 3 / 3 if lower else n * n * ntr * 128.0)
    return f


def groups_report():
    """Row groups (order="groups") against row order, DESIGN's calibration of the current
    kernel: 15.8 us per block, 58 us factor, 10 us W-product, 2.6 us hand-off.  Per case the
    modelled launch time against row order and the start gap between the two readers (i, j),
    (i + 1, j) of a column panel inside a group (rows of the last quarter, where the panels
    are long)."""
    kw = dict(c_step=15.8, c_fac=58.0, c_tri=10.0, c_pub=2.6)
    cases = [("C3 job N=32768 np=8192", 256, 65), ("C2 job N=8192 np=8192", 64, 65),
             ("POTRF N=32768", 256, 0)]
    for name, nt, ntr in cases:
        base, _ = simulate(nt, ntr, task_list(nt, ntr), **kw)
        print(f"{name:24s} rows: {base / 1e3:8.3f} ms")
        for group, skew, gmin in [(2, 0, 0), (2, 1, 0), (2, 2, 0), (2, 4, 0), (2, 4, 32), (2, 8, 0),
                                  (4, 0, 0), (4, 2, 0), (4, 4, 0), (4, 4, 32)]:
            st = {}
            tl = task_list(nt, ntr, order="groups", group=group, skew=skew, gmin=gmin)
            e, _ = simulate(nt, ntr, tl, starts=st, **kw)
            g0 = min(nt, (gmin + group - 1) // group * group)
            gaps = [abs(st[(k, i + 1, j)] - st[(k, i, j)])
                    for (k, i, j) in st
                    if i >= max(g0, 3 * nt // 4) and (i - g0) % group < group - 1
                    and (k, i + 1, j) in st and (k == "R" or j > i + 1)]
            gs = f"gap median {np.median(gaps):6.1f} us p90 {np.percentile(gaps, 90):6.1f} us" if gaps else ""
            print(f"  group={group} skew={skew} gmin={gmin:3d}: {e / 1e3:8.3f} ms "
                  f"({(e / base - 1) * 100:+.2f} %)  {gs}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c-step", type=float, default=14.8)
    ap.add_argument("--c-fac", type=float, default=48.0)
    ap.add_argument("--c-tri", type=float, default=7.4)
    ap.add_argument("--c-pub", type=float, default=1.5)
    ap.add_argument("--groups", action="store_true",
                    help="the row-group orders (GPR_DAG_RGROUP / RSKEW / RGROUP_MIN) instead")
    args = ap.parse_args()
    if args.groups:
        return groups_report()
    kw = dict(c_step=args.c_step, c_fac=args.c_fac, c_tri=args.c_tri, c_pub=args.c_pub)
    cases = [("POTRF N=8192", 64, 0), ("C2 job N=8192 np=8192", 64, 64),
             ("C3 job N=32768 np=8192", 256, 64), ("POTRF N=32768", 256, 0)]
    for name, nt, ntr in cases:
        for rlag in (0, 1, 2, 4):
            for fearly in (False, True):
                if ntr == 0 and rlag:
                    continue
                tl = task_list(nt, ntr, rlag=rlag, fearly=fearly)
                e, u = simulate(nt, ntr, tl, **kw)
                print(f"{name:26s} rlag={rlag} fearly={int(fearly)}: {e / 1e3:8.3f} ms  "
                      f"busy {u:.3f}  {flops(nt, ntr) / e / 1e6:6.1f} TF/s")


if __name__ == "__main__":
    main()
