"""NanoReviser_train.py - the counterpart of the reference's script of this name: fit the per-window tail of both models on
the device from the per-base labels an earlier `NanoReviser.py --labels` run wrote.

What is kept: -d, -S, -M / --output_model, -w / --window_size, -e, -b, --validation_split, --model_type, --model1_train_dir /
--model2_train_dir, and the names of the files under <M>/<S>/.  What is changed: --labels_from DIR replaces -r / -m graphmap
(the truth alignment is `--truth --infix --labels`' job); only the layers behind Flatten(main_out) are fitted - tensors
56 .. 59, the ones that depend on the window length and the class layout - with the 56 tensors in front frozen
(nanoreviser_amd/tailfit.py is the definition, include/nanorev.h nrv_fit_* the engine's side).  The frozen backbone runs once
per labelled window; an epoch touches 6T floats per window.  Device only: the product has no CPU forward.

--fit_depth head moves the frozen boundary back to the output of lstm4: the three per-timestep dense layers (tensors 50 .. 55)
are fitted too, a window is its 128 T lstm4 values (nanoreviser_amd/headfit.py is the definition).  The default, tail, is
everything above, byte for byte.

--fit_depth lstm4 moves it back once more, to the input of lstm4: the 256 -> 64 Bi-LSTM (tensors 44 .. 49, 164352 weights) is
fitted with the head, a window is its 256 T BatchNorm'd lstm3 values (nanoreviser_amd/lstm4fit.py is the definition).  lstm4
always starts from the loaded or continued model's own weights; --fit_init acts on the layers behind it as at head depth.

--fit_depth signal fits the part of the model that reads the raw current - conv1, conv2 and sig_dense, tensors 0, 1, 6, 7, 32 and
33 - with lstm3 (34 .. 39) and everything --fit_depth lstm4 fits; a window is its 128 T BatchNorm'd lstm2 values and its 50 T
normalised samples (nanoreviser_amd/signalfit.py is the definition, and states the two deviations: the BatchNorms inside the
fitted section stay frozen in their inference form, the reference's Dropout is applied only with --dropout).  The signal branch and lstm3 always
start from the loaded or continued model's own weights; --fit_init acts on the layers behind lstm4.  (--fit_depth lstm3 is not
offered.)

--fit_depth full fits the read branch too - lstm1 (tensors 12 .. 17) and lstm2 (22 .. 27) - with everything --fit_depth signal
fits: every tensor that is no BatchNorm's.  A window is its raw inputs, 50 T normalised samples and 6 T read features
(nanoreviser_amd/fullfit.py is the definition; the five BatchNorms stay frozen in their inference form, Dropout only with --dropout).
The four LSTMs and the signal branch start from the loaded or continued model's own weights; --fit_init acts on the layers
behind lstm4, and a fresh initialisation of the LSTMs is not offered.

--bn_reestimate (off by default; --fit_depth signal or full) re-estimates the moving statistics of the BatchNorms inside the
fitted section - three at signal depth, all five at full depth - on the device from the TRAINING rows, behind fit_begin and before
the first epoch, at the starting parameters (nanoreviser_amd/bnfit.py is the definition).  Every epoch and every validation pass
then runs on the new statistics, the written model carries them, and _summary.json gains a `bn_reestimate` entry.  gamma and beta
stay the loaded ones.  With -e 0 nothing is fitted and the loaded model is written with re-estimated statistics alone.

--fit_bn_affine (off by default; --fit_depth signal or full) fits gamma and beta of the BatchNorms inside the fitted section too:
they go in front of the parameter vector and take part in every update, each BatchNorm still applied in its inference form on
the moving statistics, which stay frozen during a step (nanoreviser_amd/bnaffine.py is the definition).  The written model
carries the fitted gamma / beta, and _summary.json gains a `bn_affine` entry: per BatchNorm the largest |change of gamma| and
|change of beta|.  With --bn_reestimate the statistics are re-estimated first, at the starting gamma / beta, then the fit runs.

--dropout RATE (0, off, by default; --fit_depth signal or full) applies the reference's Dropout behind the identity block to the
training batches, 0.2 being the reference's rate (nanoreviser_amd/dropout.py is the definition): a reproducible mask per (seed,
batch number, model, row, element), --dropout_seed (default --seed) being the seed.  The validation columns, --bn_reestimate and the
written model's forward never drop.  _summary.json gains a `dropout` entry: rate, seed and both models' final draw counters.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from typing import Optional, Sequence

import numpy as np

from . import bnaffine, bnfit, cli, fitdepth, headfit, tailfit
from .weights import load_model, load_species

HISTORY_HEAD = "epoch\tloss\tce\tcenter\tacc\tval_loss\tval_acc\tnonfinite"


def get_args(argv: Optional[Sequence[str]] = None):
    p = argparse.ArgumentParser(prog="NanoReviser_train.py", description=__doc__.split("\n\n")[0])
    p.add_argument("-d", "--fast5_base_dir", dest="fast5_base_dir", help="path to the fast5 files")
    p.add_argument("-S", "--species", dest="species", default="ecoli", help="whose weights are the frozen backbone and the starting tail")
    p.add_argument("-M", "--output_model", dest="output_model", default="./model_trained/", help="output model directory")
    p.add_argument("-w", "--window_size", dest="window_size", type=int, default=None, help="default: the loaded weights' T")
    p.add_argument("-e", "--epochs", dest="epochs", type=int, default=50)
    p.add_argument("-b", "--batch_size", dest="batch_size", type=int, default=512)
    p.add_argument("--validation_split", type=float, default=0.01,
                   help="the LAST fraction of the rows in file order, before shuffling, as Keras does")
    p.add_argument("--model_type", default="both", help="both, model1 or model2")
    p.add_argument("--model1_train_dir", default=None, help="start model 1 from a tail written by an earlier run (.f32 / .h5)")
    p.add_argument("--model2_train_dir", default=None)
    p.add_argument("--labels_from", default=None, metavar="DIR", help="required: the directory of an earlier --labels run")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--center_weight", type=float, default=tailfit.LAMBDA)
    p.add_argument("--class_weight1", default=",".join(str(int(x)) for x in tailfit.CW1), help="six weights, model 1's classes")
    p.add_argument("--class_weight2", default=",".join(str(int(x)) for x in tailfit.CW2), help="five weights, model 2's classes")
    p.add_argument("--fit_init", default="transfer", help="transfer (the loaded tail) or fresh (seeded Glorot-uniform, zero biases)")
    p.add_argument("--fit_depth", default="tail",
                   help="tail: tensors 56 .. 59 behind Flatten(main_out); head: tensors 50 .. 59 behind lstm4 (then --fit_init "
                        "fresh keeps the shipped 50 .. 55 and fresh_head draws all five layers); lstm4: tensors 44 .. 59, the "
                        "last Bi-LSTM too (it always starts from the model's own weights); signal: the signal branch (0, 1, 6, 7, "
                        "32, 33) and lstm3 (34 .. 39) in front of that, from the model's own weights; full: lstm1 (12 .. 17) and "
                        "lstm2 (22 .. 27) too - every tensor that is no BatchNorm's")
    p.add_argument("--bn_reestimate", action="store_true", default=argparse.SUPPRESS,        # (in the namespace only when given)
                   help="re-estimate the moving statistics of the BatchNorms inside the fitted section from the training rows before "
                        "the first epoch (--fit_depth signal or full); with -e 0 that alone is written")
    p.add_argument("--fit_bn_affine", action="store_true", default=argparse.SUPPRESS,        # (in the namespace only when given)
                   help="fit gamma and beta of the BatchNorms inside the fitted section too (--fit_depth signal or full)")
    p.add_argument("--dropout", type=float, default=argparse.SUPPRESS, metavar="RATE",            # (in the namespace only when given)
                   help="the reference's Dropout behind the identity block on the training batches (--fit_depth signal or full); "
                        "0.2 is the reference's rate, 0 (the default) is off")
    p.add_argument("--dropout_seed", type=int, default=argparse.SUPPRESS, help="default: --seed")
    p.add_argument("--model_dir", default=None, help="root of model/<species>/ (default: next to the package)")
    p.add_argument("-g", "--basecall_group", dest="basecall_group", default="Basecall_1D_000")
    p.add_argument("-s", "--basecall_subgroup", dest="basecall_subgroup", default="BaseCalled_template")
    p.add_argument("--reads_per_call", type=int, default=64, help="reads per device call of the feature extraction")
    return p.parse_args(argv)


def _weights(text, n, what):
    try:
        w = [float(x) for x in text.split(",")]
    except ValueError:
        w = []
    if len(w) != n or any(not np.isfinite(x) or x < 0 for x in w):
        raise ValueError(f"{what} takes {n} non-negative numbers separated by commas")
    return tuple(w)


def bn_reestimate(a) -> bool:
    """--bn_reestimate was given."""
    return bool(getattr(a, "bn_reestimate", False))


def fit_bn_affine(a) -> bool:
    """--fit_bn_affine was given."""
    return bool(getattr(a, "fit_bn_affine", False))


def dropout_rate(a) -> float:
    """--dropout's rate; 0.0, off, when it was not given."""
    return float(getattr(a, "dropout", 0.0))


def check_args(a):
    """-> the message of the first refusal, or None."""
    if not a.fast5_base_dir or not os.path.isdir(a.fast5_base_dir):
        return "-d: not a directory"
    if not a.labels_from:
        return "--labels_from DIR is required: the labels come from an earlier `NanoReviser.py --truth --infix --labels` run"
    if not os.path.isdir(a.labels_from):
        return "--labels_from: not a directory"
    if a.model_type not in ("both", "model1", "model2"):
        return "--model_type must be both, model1 or model2"
    if a.fit_depth not in _DEPTHS:
        return f"--fit_depth must be tail or head, or lstm4, or signal, or full, not {a.fit_depth!r}"
    if a.fit_depth == "tail" and a.fit_init == "fresh_head":
        return "--fit_init fresh_head draws the three dense layers behind lstm4, which --fit_depth tail does not fit"
    if a.fit_init not in (("transfer", "fresh") if a.fit_depth == "tail" else ("transfer", "fresh", "fresh_head")):
        return "--fit_init must be transfer or fresh" + (f" or fresh_head, not {a.fit_init!r}" if a.fit_depth != "tail" else "")
    if a.window_size is not None and not 1 <= a.window_size <= 32:
        return "-w must be in 1 .. 32"
    if bn_reestimate(a) and a.fit_depth not in ("signal", "full"):
        return f"--bn_reestimate: no BatchNorm lies inside the fitted section at --fit_depth {a.fit_depth} (signal and full have them)"
    if fit_bn_affine(a) and a.fit_depth not in ("signal", "full"):
        return f"--fit_bn_affine: no BatchNorm lies inside the fitted section at --fit_depth {a.fit_depth} (signal and full have them)"
    if not 0.0 <= dropout_rate(a) < 1.0:
        return "--dropout must be in [0, 1)"
    if dropout_rate(a) > 0 and a.fit_depth not in ("signal", "full"):
        return f"--dropout: the signal branch is frozen at --fit_depth {a.fit_depth}, there is nothing to drop (signal and full fit it)"
    if a.epochs < (0 if bn_reestimate(a) else 1):
        return "-e must be at least 1" + (" (0 with --bn_reestimate)" if a.epochs < 0 else "")
    if not 1 <= a.batch_size <= tailfit.MAX_BATCH:
        return f"-b must be in 1 .. {tailfit.MAX_BATCH}"
    if not 0.0 <= a.validation_split < 1.0:
        return "--validation_split must be in [0, 1)"
    if not (a.lr > 0 and np.isfinite(a.lr)) or not (a.center_weight >= 0 and np.isfinite(a.center_weight)):
        return "--lr must be positive and --center_weight non-negative"
    try:
        a.cw1, a.cw2 = _weights(a.class_weight1, 6, "--class_weight1"), _weights(a.class_weight2, 5, "--class_weight2")
    except ValueError as e:
        return str(e)
    return None


def stem(output_model, species, model_no):
    return os.path.join(output_model, species, f"{species}_win13_50ep_model{model_no}")


def _start(a, k, m, T):
    """The starting parameter vector of model k (0 / 1) and where it came from.  --fit_init and a continued run's centres act on
    the tail (at --fit_depth tail) or on tensors 50 .. 59 (at every other depth: a fresh tail keeps the shipped 50 .. 55, which do
    not depend on T, fresh_head draws all five layers); what a deeper depth fits in front of them always starts from the loaded or
    continued model's own weights."""
    fit = tailfit if a.fit_depth == "tail" else headfit
    path = (a.model1_train_dir, a.model2_train_dir)[k]
    own = m.with_window(T)
    if path:
        own = load_model(path)
        if own.T != T or own.n_class != m.n_class:
            raise ValueError(f"{path}: a model of T = {own.T} and {own.n_class} classes, expected T = {T} and {m.n_class}")
        th, how = fit.params_from_model(own), "continued"
        cen = os.path.splitext(path)[0] + "_centers.f32"
        if os.path.exists(cen):
            c = np.fromfile(cen, "<f4")
            if c.size == 16 * m.n_class:
                th[-c.size:] = c
    elif a.fit_init == "fresh_head":
        th, how = headfit.fresh_params(T, m.n_class, a.seed + k), "fresh_head"
    elif a.fit_init == "fresh" or T != m.T:
        th, how = tailfit.fresh_params(T, m.n_class, a.seed + k), "fresh"
        if fit is headfit:
            th = headfit.with_tail(headfit.params_from_model(own), th)
    else:
        th, how = fit.params_from_model(m), "transfer"
    th = th if fit is tailfit else fitdepth.start_vector(a.fit_depth, own, th)
    if fit_bn_affine(a):                                   # gamma / beta of the loaded or continued model in front
        th = np.concatenate([bnaffine.params_from_model(a.fit_depth, own)[:bnaffine.n_block(a.fit_depth)], th])
    return th, how


_DEPTHS = {d.name: d.fit for d in fitdepth.DEPTHS if d.name != "lstm3"}      # --fit_depth lstm3 is not offered


def _default_factory(a, m1, m2):
    from .engine import Reviser
    return Reviser(m1, m2, device=0)


def add_reads(a, rv, log=print):
    """Every read of -d through the host stage and its labelled windows into the engine's training set, in file order.
    -> (reads used, [(file, why)] skipped)."""
    names = sorted(f for f in os.listdir(a.fast5_base_dir) if f.endswith(".fast5"))
    used, skipped = 0, []
    for s in range(0, len(names), max(a.reads_per_call, 1)):
        jobs = [(os.path.join(a.fast5_base_dir, fn), fn, a.basecall_group, a.basecall_subgroup, False)
                for fn in names[s:s + max(a.reads_per_call, 1)]]
        entries, bundle = cli._load_bundle_labelled(jobs, False, a.labels_from)
        in_bundle = set(bundle["idx"]) if bundle is not None else set()
        for i, e in enumerate(entries):
            if i not in in_bundle:
                skipped.append((e[0], "unreadable"))
        if bundle is None:
            continue
        if "labels" not in bundle:
            skipped += [(entries[i][0], "no_bases") for i in bundle["idx"]]
            continue
        labels, flags = bundle["labels"]
        for i, f in zip(bundle["idx"], flags):
            if f == cli.SCORE_SCORED:
                used += 1
            else:
                skipped.append((entries[i][0], "stale_labels" if f == cli.SCORE_STALE else "no_labels"))
        # (a skipped read's bytes are all 0xFF: it rides along and adds no row)
        rv.fit_add_packed(rv.pack_bundle(bundle["raw"], bundle["starts"], bundle["feat"], bundle["meta"], rv.T), labels)
    for fn, why in skipped:
        log(f"[！！！Warning] {fn}: {why}; the read is not trained on")
    return used, skipped


def fit_model(a, rv, k, theta0, n_train, n_val, log=print):
    """-> (theta, history lines, the re-estimated BatchNorm statistics or None)."""
    C = 6 if k == 0 else 5
    opts = tailfit.FitOpts(B=a.batch_size, lr=a.lr, lam=a.center_weight, cw=a.cw1 if k == 0 else a.cw2)
    rv.fit_begin(k, theta0, opts)
    bn_stats = rv.fit_bn_reestimate(k, np.arange(n_train, dtype=np.uint32)) if bn_reestimate(a) else None
    val = np.arange(n_train, n_train + n_val, dtype=np.uint32)
    lines = []
    for ep in range(a.epochs):
        st = rv.fit_epoch(k, tailfit.epoch_order(n_train, a.seed, ep))
        loss, ce, cn = st.loss(opts.lam)
        if n_val:
            sv = rv.fit_eval(k, val, want_p=False)[1]
            vl, va = f"{sv.loss(opts.lam)[0]:.6f}", f"{sv.acc():.6f}"
        else:
            vl = va = "nan"
        lines.append(f"{ep + 1}\t{loss:.6f}\t{ce:.6f}\t{cn:.6f}\t{st.acc():.6f}\t{vl}\t{va}\t{st.nonfinite}")
        log(f"[s:::] model{k + 1} epoch {ep + 1}/{a.epochs}: loss {loss:.4f} acc {st.acc():.4f} val_loss {vl} val_acc {va}")
    theta, _ = rv.fit_params(k)
    assert theta.size == _DEPTHS[a.fit_depth].n_params(rv.T, C) + (bnaffine.n_block(a.fit_depth) if fit_bn_affine(a) else 0)
    return theta, lines, bn_stats


def main(argv: Optional[Sequence[str]] = None, reviser_factory=None) -> int:
    a = get_args(argv)
    bad = check_args(a)
    if bad:
        print(f"[！！！Error] {bad}", file=sys.stderr)
        return 2
    t0 = time.time()
    m1, m2 = load_species(a.species, a.model_dir)
    T = a.window_size or m1.T
    try:
        starts = [_start(a, k, m, T) for k, m in enumerate((m1, m2))]
    except (ValueError, OSError) as e:
        print(f"[！！！Error] {e}", file=sys.stderr)
        return 2
    rv = (reviser_factory or _default_factory)(a, m1.with_window(T), m2.with_window(T))
    try:
        rv.fit_reset()
        if a.fit_depth != "tail":
            rv.fit_set_depth(a.fit_depth)
        if fit_bn_affine(a):
            rv.fit_set_bn_affine(True)
        drop, drop_seed = dropout_rate(a), getattr(a, "dropout_seed", a.seed) & 0xFFFFFFFFFFFFFFFF
        if drop > 0:
            rv.fit_set_dropout(drop, drop_seed)
        used, skipped = add_reads(a, rv)
        n = rv.fit_count()
        if n == 0:
            print("[！！！Error] no labelled window: nothing to train on", file=sys.stderr)
            return 2
        n_train, n_val = tailfit.val_split(n, a.validation_split)
        if n_train == 0:
            print("[！！！Error] --validation_split leaves no row to train on", file=sys.stderr)
            return 2
        print(f"[s:::] {n} labelled windows of {used} reads ({len(skipped)} skipped): {n_train} to train on, {n_val} held out")
        os.makedirs(os.path.join(a.output_model, a.species), exist_ok=True)
        which = [k for k in (0, 1) if a.model_type in ("both", f"model{k + 1}")]
        for k in which:
            theta, lines, bn_stats = fit_model(a, rv, k, starts[k][0], n_train, n_val)
            st = stem(a.output_model, a.species, k + 1)
            m = (m1, m2)[k]
            deep = a.fit_depth != "tail"
            fit = _DEPTHS[a.fit_depth]
            nb = bnaffine.n_block(a.fit_depth) if fit_bn_affine(a) else 0
            fitted = bnaffine.fitted_model(a.fit_depth, m, theta, T) if nb else fit.fitted_model(m, theta, T)
            tailfit.write_f32(bnfit.with_stats(fitted, bn_stats) if bn_stats else fitted, st)
            fit.unpack(theta[nb:], T, m.n_class)[-1].astype("<f4").tofile(st + "_centers.f32")
            moved = {}
            for name, (sg, sb) in (bnaffine.spans(a.fit_depth).items() if nb else ()):
                d = np.abs(theta.astype(np.float64) - np.asarray(starts[k][0], np.float64))
                moved[name] = {"max_dgamma": float(d[sg].max()), "max_dbeta": float(d[sb].max())}
            d_rate, d_seed, d_draw = rv.fit_dropout() if drop > 0 else (0.0, 0, ())          # one call: the state behind this model's fit
            with open(st + "_history.tsv", "w") as fp:
                fp.write(HISTORY_HEAD + "\n" + "\n".join(lines) + "\n")
            with open(st + "_summary.json", "w") as fp:
                json.dump({"options": {"species": a.species, "window_size": T, "epochs": a.epochs, "batch_size": a.batch_size,
                                       "validation_split": a.validation_split, "seed": a.seed, "lr": a.lr,
                                       "center_weight": a.center_weight, "class_weight": list(a.cw1 if k == 0 else a.cw2),
                                       "init": starts[k][1], "labels_from": os.path.abspath(a.labels_from),
                                       **({"fit_depth": a.fit_depth} if deep else {}),
                                       **({"fit_bn_affine": True} if nb else {}),
                                       **({"dropout": drop, "dropout_seed": drop_seed} if drop > 0 else {})},
                           **({"dropout": {"rate": d_rate, "seed": d_seed, "draw": list(d_draw)}} if drop > 0 else {}),
                           **({"bn_affine": moved} if nb else {}),
                           **({"bn_reestimate": bnfit.drift(bnfit.bn_of(m), bn_stats)} if bn_stats else {}),
                           "rows": n, "train_rows": n_train, "val_rows": n_val, "reads": used,
                           "skipped_reads": [list(s) for s in skipped], "seconds": round(time.time() - t0, 3)}, fp, indent=1)
                fp.write("\n")
    finally:
        rv.close()
    return 0
