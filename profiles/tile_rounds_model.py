#!/usr/bin/env python3
"""CPU model of the loop structure of k_fluid_tiled's fluid pass (CellMode=full): how many
candidate-test groups, drain rounds and drain iterations a wave runs, from the particle
positions alone.  numpy only; the particles come from dualsphysics_multilayer_amd/case.py.

  python3 profiles/tile_rounds_model.py [--dp 0.0045] [--stride 8] [--jitter 0.35] [--seed 1]

It follows the kernel's own structure (csrc/sph_items.hpp, sph_tiled.hpp,
sph_interaction_tiled.hip):
  * fluid particles in cell order, items of <= 128 particles of one cell row, cut at a 5th
    x-cell; the item's two waves split as lane_order does;
  * per drain unit (four point-mirrored row pairs, then the own row) each lane's two 3-cell
    windows and its accepted candidates at 1.0001 (2h)^2;
  * a round tests each window in groups of 32 records (a group runs when any lane of the
    wave has records left in it) and drains the accepted bits word by word, two per
    iteration, for as long as the wave's busiest lane.

Printed: the window-length histogram, rounds per wave-unit, groups tested per wave-unit,
the drain's lane utilisation, and the modelled VALU wave-instructions of the variants
relative to today's kernel (cost constants: 165 per 32-record group, 115 per drain
iteration, 80 per round; A: the last group in 8-record steps; B: rounds of 192 per window,
+6 per iteration for the six-word chain, on every unit or only where a lane's window
exceeds 128; one round per unit at no extra cost as the bound).  `--stride k` takes every
k-th item (the lattice repeats); `--jitter j` moves every particle by up to +-j dp per axis
first (a disordered flow).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dualsphysics_multilayer_amd.case import DamBreakCase  # noqa: E402

TB, TMAXCELLS = 128, 4
C_GROUP, C_ITER, C_ROUND, C_CHAIN6 = 165.0, 115.0, 80.0, 6.0
UNITS = ((-1, -1), (-1, 1), (-1, 0), (0, -1), (0, 0))  # (dz, dy) of row a; row b its mirror


def word_iters(acc, start, length, lo, hi, wbits):
    """Per lane, sum over the words of `wbits` candidates of window records [lo, hi) (relative
    to the window start) of ceil(bits / 2).  acc: [lanes, records] accepted, start/length the
    lanes' windows in record indices."""
    n, m = acc.shape
    k = np.arange(m)[None, :] - start[:, None]
    it = np.zeros(n, np.int64)
    for w0 in range(lo, hi, wbits):
        inw = (k >= w0) & (k < min(w0 + wbits, hi)) & (k < length[:, None])
        it += ((acc & inw).sum(axis=1) + 1) // 2
    return it


def model(case, stride, variants):
    dp = case.dp
    h = float(np.float32(case.h))
    scell = float(np.float32(2.0 * h))
    ks2 = np.float32(scell) ** 2 * 1.0001
    lo, _ = case.map_limits()
    pos = case.pos[case.npb:]
    c = np.floor((pos - lo) / scell).astype(np.int64)
    ncx, ncy, ncz = (int(v) + 1 for v in c.max(axis=0))
    order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))
    pos, c = pos[order], c[order]
    rel = pos - lo - c * scell
    hist = np.zeros((ncz, ncy, ncx), np.int64)
    np.add.at(hist, (c[:, 2], c[:, 1], c[:, 0]), 1)
    pre = np.concatenate([np.zeros((ncz, ncy, 1), np.int64), hist.cumsum(axis=2)], axis=2)
    rowstart = np.concatenate([[0], hist.sum(axis=2).ravel().cumsum()])  # first particle of row z*ncy+y
    hs = 0.5 * scell
    tot = {v: 0.0 for v in variants}
    stat = dict(units=0, rounds=0, second=0, groups=0, groups_a=0.0, it_sum=0, it_max=0, it1_sum=0, it1_max=0)
    whist = {}
    item = -1
    for cz in range(ncz):
        for cy in range(ncy):
            pr = pre[cz, cy]
            p, pend, cc = 0, int(pr[ncx]), 0
            r0 = rowstart[cz * ncy + cy]
            while p < pend:
                while pr[cc + 1] <= p:
                    cc += 1
                q = int(min(p + TB, pend, pr[min(cc + TMAXCELLS, ncx)]))
                e = cc
                while pr[e + 1] < q:
                    e += 1
                p0, p = p, q
                item += 1
                if item % stride:
                    continue
                sel = np.arange(r0 + p0, r0 + q)
                low = np.abs(rel[sel, 1] - hs) + np.abs(rel[sel, 2] - hs) < hs
                sel = sel[np.concatenate([np.nonzero(low)[0], np.nonzero(~low)[0]])]
                xa, xb = max(cc - 1, 0), min(e + 1, ncx - 1)
                lxa, lxb = np.maximum(c[sel, 0] - 1, 0), np.minimum(c[sel, 0] + 1, ncx - 1)
                for u, (dz, dy) in enumerate(UNITS):
                    win = []
                    for k in range(2 if u < 4 else 1):
                        z, y = cz + (-dz if k else dz), cy + (-dy if k else dy)
                        if z < 0 or z >= ncz or y < 0 or y >= ncy:
                            continue
                        r = pre[z, y]
                        rs, re = int(r[xa]), int(r[xb + 1])
                        if re == rs:
                            continue
                        rec = rowstart[z * ncy + y] + np.arange(rs, re)
                        d = pos[sel][:, None, :] - pos[rec][None, :, :]
                        acc = np.einsum("ijk,ijk->ij", d, d).astype(np.float32) <= ks2
                        win.append((acc, r[lxa] - rs, r[lxb + 1] - r[lxa]))
                    if not win:
                        continue
                    for acc, st, ln in win:
                        for v, cnt in zip(*np.unique(ln, return_counts=True)):
                            whist[int(v)] = whist.get(int(v), 0) + int(cnt)
                    for wv in range((len(sel) + 63) // 64):
                        ws = slice(64 * wv, 64 * wv + 64)
                        lens = [ln[ws] for _, _, ln in win]
                        longest = max(int(x.max()) for x in lens)
                        if longest == 0:
                            continue

                        def cost(rsize, a_groups, chain6, rsize_if_long=None):
                            rs_ = rsize
                            if rsize_if_long is not None and longest > 128:
                                rs_ = rsize_if_long
                            six = chain6 and rs_ > 128  # the longer chain costs every iteration of the unit
                            rs_ = min(rs_, -(-longest // 64) * 64)  # (one round: as long as the unit needs)
                            t, rounds, groups, its, itm = 0.0, 0, 0.0, 0, 0
                            for off in range(0, longest, rs_):
                                rounds += 1
                                it = np.zeros(len(lens[0]), np.int64)
                                for (acc, st, ln), l in zip(win, lens):
                                    left = np.clip(l - off, 0, rs_)
                                    for g in range(0, rs_, 32):
                                        m = int(np.clip(left - g, 0, 32).max())
                                        if m:
                                            groups += (-(-m // 8)) / 4.0 if a_groups else 1.0
                                    it += word_iters(acc[ws], st[ws], ln[ws], off, off + rs_, 64)
                                its += int(it.sum())
                                itm += int(it.max())
                                t += C_ROUND + int(it.max()) * (C_ITER + (C_CHAIN6 if six else 0.0))
                            return t + groups * C_GROUP, rounds, groups, its, itm

                        t0, rounds, groups, its, itm = cost(128, False, False)
                        tot["today"] += t0
                        stat["units"] += 1
                        stat["rounds"] += rounds
                        stat["second"] += rounds > 1
                        stat["groups"] += groups
                        stat["it_sum"] += its
                        stat["it_max"] += itm
                        ta, _, ga, _, _ = cost(128, True, False)
                        tot["A"] += ta
                        stat["groups_a"] += ga
                        tot["B"] += cost(192, False, True)[0]
                        tot["A+B"] += cost(192, True, True)[0]
                        tot["A+B where > 128"] += cost(128, True, True, 192)[0]
                        tb, _, _, its1, itm1 = cost(1 << 20, True, False)
                        # one round: groups only as far as the windows reach
                        tot["A+one round"] += tb
                        stat["it1_sum"] += its1
                        stat["it1_max"] += itm1
    return tot, stat, whist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dp", type=float, default=0.0045)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--jitter", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    case = DamBreakCase(a.dp)
    if a.jitter:
        rng = np.random.default_rng(a.seed)
        case.pos = case.pos.copy()
        case.pos[case.npb:] += rng.uniform(-a.jitter, a.jitter, (case.np - case.npb, 3)) * a.dp
    variants = ("today", "A", "B", "A+B", "A+B where > 128", "A+one round")
    tot, st, whist = model(case, a.stride, variants)
    n = sum(whist.values())
    print("particles %d, every %d-th item, jitter %.2f dp" % (case.np, a.stride, a.jitter))
    print("window length: share of (particle, row) windows")
    for v, cnt in sorted(whist.items(), key=lambda kv: -kv[1])[:10]:
        print("  %4d  %5.1f %%" % (v, 100.0 * cnt / n))
    print("  > 128: %.1f %%   > 192: %.1f %%" % (100.0 * sum(c for v, c in whist.items() if v > 128) / n,
                                                 100.0 * sum(c for v, c in whist.items() if v > 192) / n))
    print("wave-units %d: rounds per unit %.3f, with a second round %.1f %%" %
          (st["units"], st["rounds"] / st["units"], 100.0 * st["second"] / st["units"]))
    print("groups tested per wave-unit %.2f (last group in 8-record steps: %.2f, -%.1f %%)" %
          (st["groups"] / st["units"], st["groups_a"] / st["units"], 100.0 * (1 - st["groups_a"] / st["groups"])))
    print("drain lane utilisation %.3f (one round per unit: %.3f)" %
          (st["it_sum"] / (64.0 * st["it_max"]), st["it1_sum"] / (64.0 * st["it1_max"])))
    print("test share of today's modelled instructions %.1f %%" % (100.0 * st["groups"] * C_GROUP / tot["today"]))
    print("modelled VALU wave-instructions relative to today")
    for v in variants:
        print("  %-18s %.3f" % (v, tot[v] / tot["today"]))


if __name__ == "__main__":
    main()
