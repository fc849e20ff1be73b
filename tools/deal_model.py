"""Measurement aid (CPU): fit the time model of the forward tile launch's compute units that the deal (csrc/gsr_common.h: deal_term,
build_tile_order_model) uses, from per-tile stamps recorded on the device, and judge it on deals it was not fitted on.

Recording (GPU box; tools/phase_stamps.py, stamped build):
  PS_DUMP=out.npz PS_DEALS=random:24 python tools/phase_stamps.py label      shipped deal + 24 random deals of each XCD's tiles
  PS_DUMP=out.npz PS_DEALS=deals.npz ...                                      the tables in deals.npz["orders"] (n, tiles)
A table is imposed through the hint: the builder sorts by the previous call's tile_total, so writing ranks there places any tile on
any workgroup with the shipped kernels - a candidate deal is measured before any device code exists for it.

What the stamps say (profiles/r11_deal_model.md): the four tiles of a compute unit start AND end in the order of their de-phase slots
(slot = workgroup >> 8); the slot-3 tile ended last on 256 of 256 units.  An event model in which the resident tiles share the unit
equally (the per-batch times of tools/micro/blend_mix_bench.hip at W = 1 ... 4) does not describe that: fitted to the stamps its
rates come out negative.  What does: the unit's end as a LINEAR function of each slot's batches and list length,
    end = sum_s wn[s] x batches[s] + wl[s] x list_length[s] + c,
fitted by least squares on the odd-numbered deals and judged on the even-numbered ones.

usage: python tools/deal_model.py fit out.npz [more.npz ...]         coefficients (us and the header's 2^-16 us integers), held-out fit
       python tools/deal_model.py search out.npz deals_out.npz      tables for PS_DEALS: shipped, and the exchange search at 8 / 32 / 400 passes
"""
from __future__ import annotations

import sys

import numpy as np


def corr(a, b):
    return float(np.corrcoef(a, b)[0, 1])


def load(paths):
    """-> rows: one dict per stamped call with a hinted deal (deal id unique across files), per-slot features of its 256 units."""
    rows, upc = [], {}
    for fi, path in enumerate(paths):
        z = np.load(path)
        nb, ln = np.ceil(z["walked"] / 32.0), z["list_length"].astype(float)
        for c, r in enumerate(z["recs"]):
            d = int(z["deal_of_rec"][c])
            t0 = r[:, 1].min()
            tile_of = np.zeros(len(r), int)
            tile_of[r[:, 0].astype(int)] = np.arange(len(r))
            t = tile_of.reshape(4, -1)  # [slot, workgroup & 255]: the tiles that share a compute unit
            cu = r[:, 4][t]
            rows.append(dict(deal=(fi, d), hinted=d > 0, NB=nb[t], LN=ln[t], end=(r[:, 3] - t0)[t].max(0), last=(r[:, 3] - t0)[t].argmax(0),
                             as_dealt=bool((cu == cu[0]).all())))
            upc[(fi, d)] = float(z["us_per_call"][d])
    return rows, upc


def feats(r):
    return np.concatenate([r["NB"].T, r["LN"].T, np.ones((r["NB"].shape[1], 1))], 1)


def fit(rows):
    deals = sorted({r["deal"] for r in rows if r["hinted"]})
    train = {d for i, d in enumerate(deals) if i % 2 == 1}
    tr = [r for r in rows if r["deal"] in train]
    te = [r for r in rows if r["hinted"] and r["deal"] not in train]
    w = np.linalg.lstsq(np.concatenate([feats(r) for r in tr]), np.concatenate([r["end"] for r in tr]), rcond=None)[0]
    return w, tr, te


def cmd_fit(paths):
    rows, upc = load(paths)
    w, tr, te = fit(rows)
    print(f"{len(rows)} stamped calls, {len({r['deal'] for r in rows})} deals; compute units that hold workgroups b, b + 256, b + 512, b + 768: "
          f"{sum(r['as_dealt'] for r in rows)} of {len(rows)} calls all 256")
    print("slot whose tile ends last on its unit (units, all calls):", np.bincount(np.concatenate([r["last"] for r in rows]), minlength=4))
    print("us per batch by slot", np.round(w[:4], 4), "| us per list entry by slot", np.round(w[4:8], 6), "| constant", round(float(w[8]), 3))
    print("  as integers of 2^-16 us: per walked entry", np.round(w[:4] * 65536 / 32).astype(int), "per list entry", np.round(w[4:8] * 65536).astype(int))
    for name, rs in (("fitted on", tr), ("held out", te)):
        cm = [corr(feats(r) @ w, r["end"]) for r in rs]
        cb = [corr(r["NB"].sum(0), r["end"]) for r in rs]
        rms = np.sqrt(np.mean([(feats(r) @ w - r["end"]) ** 2 for r in rs]))
        print(f"  {name}: {len(rs)} calls; per call corr(unit end, model) mean {np.mean(cm):.3f} min {np.min(cm):.3f} | corr(unit end, batch sum) mean {np.mean(cb):.3f} "
              f"min {np.min(cb):.3f} | rms {rms:.3f} us")
    by = {}
    for r in te:
        by.setdefault(r["deal"], []).append(((feats(r) @ w).max(), r["end"].max(), r["NB"].sum(0).max()))
    m = np.array([np.mean(v, 0) for v in by.values()])
    u = np.array([upc[d] for d in by])
    print(f"  across the {len(by)} held-out deals: corr(modelled slowest unit, stamped end of the launch) {corr(m[:, 0], m[:, 1]):.3f}, with the forward's us per call "
          f"{corr(m[:, 0], u):.3f}; the largest batch sum's {corr(m[:, 2], m[:, 1]):.3f} and {corr(m[:, 2], u):.3f}")
    return w


def search(order, nb, ln, w, passes):
    """The header's exchange search in floating point (workgroup k of an XCD: slot k >> 5, unit k & 31); order: tile of each workgroup."""
    o = order.copy()
    term = lambda s, t: w[s] * nb[t] + w[4 + s] * ln[t]
    for x in range(8):
        for _ in range(passes):
            t = o[x::8]
            cnt = len(t)
            cost = np.zeros(32)
            for k in range(cnt):
                cost[k & 31] += term(k >> 5, t[k])
            worst = int(cost.argmax())
            best, pick = cost[worst] - 1e-9, None
            for k in range(cnt):
                if (k & 31) == worst:
                    continue
                for sa in range(4):
                    ka = 32 * sa + worst
                    if ka >= cnt:
                        continue
                    m = max(cost[worst] - term(sa, t[ka]) + term(sa, t[k]), cost[k & 31] - term(k >> 5, t[k]) + term(k >> 5, t[ka]))
                    if m < best:
                        best, pick = m, (k, ka)
            if pick is None:
                break
            ia, ib = 8 * pick[0] + x, 8 * pick[1] + x
            o[ia], o[ib] = o[ib], o[ia]
    return o


def cmd_search(path, out):
    rows, _ = load([path])
    w, _, _ = fit(rows)
    z = np.load(path)
    nb, ln = np.ceil(z["walked"] / 32.0), z["list_length"].astype(float)
    r0 = z["recs"][0]  # (the first record is the shipped deal's)
    shipped = np.zeros(len(r0), np.int64)
    shipped[r0[:, 0].astype(int)] = np.arange(len(r0))
    unit_max = lambda o: float((feats(dict(NB=nb[o.reshape(4, -1)], LN=ln[o.reshape(4, -1)])) @ w).max())
    orders = []
    print("modelled slowest unit: shipped", round(unit_max(shipped), 3))
    for _ in range(3):  # (three turns each: the first loops of a process read slow)
        orders.append(shipped)
        for p in (8, 32, 400):
            orders.append(search(shipped, nb, ln, w, p))
    for p, o in zip((8, 32, 400), orders[1:4]):
        print(f"  after {p} passes per XCD: {unit_max(o):.3f} ({int((o != shipped).sum()) // 2} exchanges)")
    np.savez(out, orders=np.array(orders))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "fit":
        cmd_fit(sys.argv[2:])
    elif len(sys.argv) == 4 and sys.argv[1] == "search":
        cmd_search(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
