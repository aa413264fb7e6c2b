#!/usr/bin/env python3
"""Time nrv_fit_epoch at the six fit depths (tail: tensors 56 .. 59; head: tensors 50 .. 59; lstm4: tensors 44 .. 59; lstm3:
tensors 34 .. 39 and 44 .. 59; signal: tensors 0, 1, 6, 7, 32 .. 39 and 44 .. 59; full: every tensor that is no BatchNorm's) on the device.  A plain script: it takes no part in bench.py and sets no bar.

A set of seeded rows goes in through the unit doors (nrv_fit_set_rows / _head / _lstm4 / _lstm3 / _signal / _full), so the frozen backbone never
runs: what is timed is one whole nrv_fit_epoch call - the upload of the row order, every batch's launches enqueued back to back
and the one synchronise at the end - by a host clock around the call, which returns only after that synchronise.  Per depth:
untimed epochs first (first launches load code objects and size the scratch buffers), then --repeats timed epochs; the median
and the spread (min .. max) are printed as rows/s, then one JSON line with everything.

    python tools/fit_bench.py [--rows 65536] [-b 512] [-w 11] [--warmup 3] [--repeats 9] [--model 0] [--depths tail,head,lstm4,lstm3,signal,full]

--bn_reestimate times nrv_fit_bn_reestimate over all rows instead of the epoch (depths lstm3, signal and full; give them with
--depths), by the same protocol, and in the same process nrv_fit_eval over the same rows as the yardstick: the rate in rows/s and
the ratio of a re-estimation to its number of passes (three at signal and full depth, one at lstm3 depth) x one nrv_fit_eval.

--bn_affine times the epoch twice per depth in the same process (depths lstm3, signal and full; give them with --depths): with
nrv_fit_set_bn_affine off, then on - gamma and beta of the BatchNorms inside the fitted section in front of the vector, from the
model's own - by the same protocol, and prints the switch-on figure with the switch-off one next to it.

--dropout RATE times the epoch twice per depth in the same process (depths signal and full; give them with --depths): with
nrv_fit_set_dropout off, then on at RATE (seed --seed) from the same start, by the same protocol, and prints the switch-on figure
with the switch-off one next to it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def flop_per_row(depth, T, C):
    """Multiply-adds x 2 the algorithm needs per row and batch: forward once, data and weight gradients; at head depth the
    kernel's recomputation of the two wide forward products is NOT counted (it is the implementation's choice)."""
    tail = 2 * (96 * T + 16 * C) * 3
    mlp = 2 * T * (128 * 128 + 128 * 32 + 32 * 6)
    if depth == "tail":
        return tail
    if depth == "head":
        return tail + 3 * mlp - 2 * T * 128 * 128          # (no data gradient into X)
    # lstm4 depth: the head with its data gradient dX4 = dh1 W1^T; per direction the input and recurrent products forward, the
    # recurrent data gradient dz U^T (none into Xb: lstm3 is frozen) and the two weight-gradient products
    lstm = 2 * T * 2 * (256 * 256 + 64 * 256)
    l4 = tail + 3 * mlp + 2 * lstm + 2 * T * 2 * 64 * 256
    if depth == "lstm4":
        return l4
    # lstm3 depth: the lstm4 depth with its data gradient dXb4 = dz4 W4^T; lstm3's two forward products, its recurrent data
    # gradient and its two weight-gradient products, per direction
    lstm3 = 2 * T * 2 * (192 * 512 + 128 * 512)
    l3 = l4 + 2 * T * 2 * 256 * 256 + 2 * lstm3 + 2 * T * 2 * 128 * 512
    if depth == "lstm3":
        return l3
    # signal depth: the lstm3 depth with the 64 signal columns of dXin = dz3 W3^T (both directions); per (row, t) the two
    # convolutions and the 400 -> 64 product forward, gWs = F^T dS, dF = dS Ws^T, conv2's weight and data gradient and conv1's
    # weight gradient; the backward launch's recomputation of a1, c1 and a2 is NOT counted
    conv1, conv2, dense = 50 * 8 * 3, 50 * 8 * 24, 400 * 64
    sg = l3 + 2 * T * (2 * 512 * 64 + (conv1 + conv2 + dense) + 2 * dense + 2 * conv2 + conv1)
    if depth == "signal":
        return sg
    # full depth: the signal depth with the other 128 columns of dXin; per direction lstm2's two forward products, its
    # recurrent data gradient, its two weight-gradient products and its data gradient dz2 W2^T; the same of lstm1 without a data
    # gradient into the features
    lstm2, lstm1 = 2 * T * 2 * (32 * 256 + 64 * 256), 2 * T * 2 * (6 * 64 + 16 * 64)
    return (sg + 2 * T * 2 * 512 * 128 + 2 * lstm2 + 2 * T * 2 * (64 * 256 + 32 * 256) + 2 * lstm1 + 2 * T * 2 * 16 * 64)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("-b", "--batch_size", type=int, default=512)
    ap.add_argument("-w", "--window_size", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--model", type=int, default=0, choices=(0, 1))
    ap.add_argument("--species", default="ecoli")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--depths", default="tail,head,lstm4,lstm3", help="the depths to time, in this order (signal and full are not in the default)")
    ap.add_argument("--bn_reestimate", action="store_true", help="time nrv_fit_bn_reestimate against nrv_fit_eval instead of the epoch")
    ap.add_argument("--bn_affine", action="store_true", help="time the epoch with nrv_fit_set_bn_affine off, then on, in one process")
    ap.add_argument("--dropout", type=float, default=0.0, metavar="RATE",
                    help="time the epoch with nrv_fit_set_dropout off, then on at RATE, in one process (0.2 is the reference's rate)")
    a = ap.parse_args(argv)
    if not 0.0 <= a.dropout < 1.0:
        ap.error("--dropout must be in [0, 1)")
    if a.dropout > 0 and (a.bn_affine or a.bn_reestimate):
        ap.error("--dropout with --bn_affine or --bn_reestimate: one comparison per run (each times its own switch against the plain epoch)")
    frozen = [d for d in a.depths.split(",") if d not in ("signal", "full")]
    if a.dropout > 0 and frozen:
        ap.error(f"--dropout: the signal branch is frozen at depth {', '.join(frozen)}, there is nothing to drop (give --depths signal,full)")
    from nanoreviser_amd import bnaffine, bnfit, fitdepth, headfit, tailfit
    from nanoreviser_amd.engine import Reviser
    from nanoreviser_amd.weights import load_species
    T, k, n = a.window_size, a.model, a.rows
    C = 6 - k
    m1, m2 = load_species(a.species)
    rv = Reviser(m1.with_window(T), m2.with_window(T), device=0)            # no device: this raises, there is no fallback
    rng = np.random.default_rng(a.seed)
    y1, y2 = rng.integers(0, 6, n).astype(np.uint8), rng.integers(0, 5, n).astype(np.uint8)
    opts = tailfit.default_opts(k, B=a.batch_size)
    out = {"rows": n, "B": a.batch_size, "T": T, "model": k, "warmup": a.warmup, "repeats": a.repeats, "device": None}
    try:
        import torch
        out["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    try:
        for depth in a.depths.split(","):
            rv.fit_reset()
            rv.fit_set_depth(depth)
            d = fitdepth.BY_NAME[depth]
            # seeded rows of the depth's shapes, a per-model array the same for both models: non-negative like main_out's values
            # at tail depth, inside (-1, 1) like lstm4's outputs at head depth, standard normal at the others
            draw = {"tail": lambda sh: np.maximum(rng.normal(0, 1, sh), 0), "head": lambda sh: np.clip(rng.normal(0, 0.5, sh), -0.999, 0.999)}
            xs = []
            for r in d.rows:
                xs += [draw.get(depth, lambda sh: rng.normal(0, 1, sh))((n,) + r.shape(T)).astype(np.float32)] * len(r.args)
            getattr(rv, "fit_set_rows" + d.suffix)(*xs, y1, y2)
            # a fresh tail at tail depth; at the others a fresh head behind the shipped model's own weights (the LSTMs and the
            # signal branch have no fresh start)
            fresh = tailfit.fresh_params(T, C, a.seed) if depth == "tail" else headfit.fresh_params(T, C, a.seed)
            th = fitdepth.start_vector(depth, (m1, m2)[k].with_window(T), fresh)
            rv.fit_begin(k, th, opts)
            if a.bn_reestimate:
                rows = np.arange(n, dtype=np.uint32)
                passes = len(bnfit.stages(depth))
                calls = {"eval": lambda: rv.fit_eval(k, rows, want_p=False), "bn_reestimate": lambda: rv.fit_bn_reestimate(k, rows)}
                secs = {}
                for name, call in calls.items():           # nrv_fit_eval first: its kernels read the handle's statistics either way
                    for _ in range(a.warmup):
                        call()
                    t = []
                    for _ in range(a.repeats):
                        t0 = time.perf_counter()
                        call()                             # both return after the stream's synchronise
                        t.append(time.perf_counter() - t0)
                    secs[name] = np.array(t)
                ev, bn = secs["eval"], secs["bn_reestimate"]
                ratio = bn / (passes * np.median(ev))
                out[depth] = {"passes": passes, "eval_ms_median": float(np.median(ev) * 1e3), "eval_ms_min": float(ev.min() * 1e3),
                              "eval_ms_max": float(ev.max() * 1e3), "bn_ms_median": float(np.median(bn) * 1e3),
                              "bn_ms_min": float(bn.min() * 1e3), "bn_ms_max": float(bn.max() * 1e3),
                              "bn_rows_per_s_median": float(np.median(n / bn)), "bn_rows_per_s_min": float((n / bn).min()),
                              "bn_rows_per_s_max": float((n / bn).max()), "ratio_to_eval_passes_median": float(np.median(ratio)),
                              "ratio_to_eval_passes_min": float(ratio.min()), "ratio_to_eval_passes_max": float(ratio.max())}
                print(f"{depth}: nrv_fit_bn_reestimate {np.median(n / bn):,.0f} rows/s (min {(n / bn).min():,.0f}, max {(n / bn).max():,.0f}), "
                      f"{np.median(bn) * 1e3:.2f} ms; nrv_fit_eval {np.median(ev) * 1e3:.2f} ms (min {ev.min() * 1e3:.2f}, max "
                      f"{ev.max() * 1e3:.2f}); ratio to {passes} x eval {np.median(ratio):.3f} (min {ratio.min():.3f}, max {ratio.max():.3f})")
                continue
            def epochs():
                for ep in range(a.warmup):
                    rv.fit_epoch(k, tailfit.epoch_order(n, a.seed, ep))
                secs = []
                for ep in range(a.repeats):
                    order = tailfit.epoch_order(n, a.seed, a.warmup + ep)
                    t0 = time.perf_counter()
                    st = rv.fit_epoch(k, order)            # returns after the stream's synchronise
                    secs.append(time.perf_counter() - t0)
                    assert st.rows == n and st.nonfinite == 0, st
                return np.array(secs)
            secs = epochs()
            if a.bn_affine:                                # the same rows and start with the block in front, in the same process
                off = secs
                rv.fit_set_bn_affine(True)
                nb = bnaffine.n_block(depth)
                th = np.concatenate([bnaffine.params_from_model(depth, (m1, m2)[k].with_window(T))[:nb], th])
                rv.fit_begin(k, th, opts)
                secs = epochs()
                nbat = -(-n // a.batch_size)
                print(f"{depth}: switch off {np.median(n / off):,.0f} rows/s, {np.median(off) / nbat * 1e6:.1f} us per batch (epoch "
                      f"{np.median(off) * 1e3:.2f} ms, min {off.min() * 1e3:.2f}, max {off.max() * 1e3:.2f}); switch on, {nb} more parameters, "
                      f"x {np.median(secs) / np.median(off):.4f}:")
            if a.dropout > 0:                              # the same rows and start with the switch on, in the same process
                off = secs
                rv.fit_set_dropout(a.dropout, a.seed)
                rv.fit_begin(k, th, opts)
                secs = epochs()
                nbat = -(-n // a.batch_size)
                assert rv.fit_dropout()[2][k] == nbat * (a.warmup + a.repeats)
                print(f"{depth}: switch off {np.median(n / off):,.0f} rows/s, {np.median(off) / nbat * 1e6:.1f} us per batch (epoch "
                      f"{np.median(off) * 1e3:.2f} ms, min {off.min() * 1e3:.2f}, max {off.max() * 1e3:.2f}); dropout {a.dropout:g} on, "
                      f"x {np.median(secs) / np.median(off):.4f}:")
            rate = n / secs
            gf = flop_per_row(depth, T, C) * 1e-9
            out[depth] = {"params": int(th.size), "batches": -(-n // a.batch_size), "epoch_ms_median": float(np.median(secs) * 1e3),
                          "epoch_ms_min": float(secs.min() * 1e3), "epoch_ms_max": float(secs.max() * 1e3),
                          "rows_per_s_median": float(np.median(rate)), "rows_per_s_min": float(rate.min()),
                          "rows_per_s_max": float(rate.max()), "gflop_per_batch": gf * a.batch_size,
                          "gflop_per_s_median": float(np.median(rate) * gf)}
            if a.dropout > 0:
                out[depth].update(dropout=a.dropout, off_epoch_ms_median=float(np.median(off) * 1e3), off_epoch_ms_min=float(off.min() * 1e3),
                                  off_epoch_ms_max=float(off.max() * 1e3), off_rows_per_s_median=float(np.median(n / off)),
                                  on_over_off_median=float(np.median(secs) / np.median(off)))
            if a.bn_affine:
                out[depth].update(bn_affine=True, off_epoch_ms_median=float(np.median(off) * 1e3), off_epoch_ms_min=float(off.min() * 1e3),
                                  off_epoch_ms_max=float(off.max() * 1e3), off_rows_per_s_median=float(np.median(n / off)),
                                  on_over_off_median=float(np.median(secs) / np.median(off)))
            print(f"{depth}: {np.median(rate):,.0f} rows/s (min {rate.min():,.0f}, max {rate.max():,.0f}); epoch of {n} rows in "
                  f"{np.median(secs) * 1e3:.2f} ms = {np.median(secs) / out[depth]['batches'] * 1e6:.1f} us per batch of {a.batch_size}; "
                  f"{out[depth]['gflop_per_s_median']:,.0f} GFLOP/s of the algorithm's own operations")
    finally:
        rv.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
