#!/usr/bin/env python
"""Per-sample error of WaveNet scoring against the float64 checker, for every case, window and utterance of tests/score_cases.py:
e = max|nll - nll64| / max|nll64| for the HIP path (e_hip) and for the float32 torch run of the same lines (e_t32), the ratio, and
the held-out loss beside the float64 and float32 means.  Writes --out (default profiles/wavenet_score_parity.txt).  Needs the GPU.
--wide: the cases of tests/score_wide_cases.py instead (residual = dilation width 64 and 128), first their width-32 twins: the NLL
errors and, through twv_wavenet_score_view after the first window batch, e of every layer's z rows and of the raw output; the worst
width-32 e_z fixes floor_z (default --out profiles/wavenet_score_wide_parity.txt)."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import score_cases as SC
import twvk_amd
from twvk_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--wide", action="store_true")
args = ap.parse_args()
args.out = args.out or os.path.join(ROOT, "profiles", "wavenet_score_wide_parity.txt" if args.wide else "wavenet_score_parity.txt")
assert torch.cuda.is_available(), "a measurement needs the GPU"


def wide():
    import score_wide_cases as WC
    lines = ["WaveNet scoring at residual = dilation width 64 and 128 (sc_layer_wide_fwd_kernel) and the width-32 twins of the same cases",
             "(sc_layer_fwd_kernel, untouched), against the float64 torch restatement (scripts/score_parity.py --wide)",
             "library %s on %s" % (_lib.lib().twv_version().decode(), torch.cuda.get_device_name(0)),
             "nll: e = max|nll - nll64| / max|nll64|, worst utterance and window, whole utterances; bar e_hip <= max(%g * e_t32, %g)" % (SC.RATIO, SC.FLOOR),
             "z, y: through twv_wavenet_score_view after the first window batch, against the checker on each live slot's crop;",
             "      e = max|. - .64| / max|.64| per layer over the live slots (z) and per slot (y), the worst of them shown", "",
             "%-24s %5s %10s %10s %10s %10s %10s %10s %13s %13s  %s" % ("case", "width", "nll e_hip", "nll e_t32", "z e_hip", "z e_t32", "y e_hip", "y e_t32", "held-out", "float64 mean", "route")]
    worst32 = 0.0
    table = {}
    for width in (32, None):
        for cid in WC.IDS:
            c = WC.case(cid, width)
            n64, n32 = WC.reference(cid, width)
            en = (0.0, 0.0)
            for wf in c.windows:
                sc = c.scorer(wf)
                for i, g in enumerate(sc.score(c.audios, c.mels, c.gcs)):
                    e = SC.errors(g.cpu().numpy(), n64[i], n32[i])
                    en = max(en, e)
            sc = c.scorer()
            r = sc.route()
            rows = WC.first_batch(c)
            sc.run(*sc.stage(rows, c.audios, c.mels, c.gcs))
            ez, ey = WC.view_errors(c, sc, rows)
            wz, wy = max(ez.values()), max(ey.values())
            loss, _ = sc.held_out_loss(c.audios, c.mels, c.gcs)
            table[c.id] = (en, wz, wy)
            if width == 32:
                worst32 = max(worst32, wz[0], wy[0])
            lines.append("%-24s %5d %10.3e %10.3e %10.3e %10.3e %10.3e %10.3e %13.9f %13.9f  lc=%s head=%s loss=%s" % (
                c.id, c.W, en[0], en[1], wz[0], wz[1], wy[0], wy[1], loss, WC.means(cid, width)[0], r["lc"], r["head"], r["loss"]))
    floor_z = max(5e-6, 2 * worst32)
    lines += ["", "worst e of z and y of the width-32 kernel through the view: %.3e" % worst32,
              "floor_z = max(5e-6, 2 x %.3e) = %.3g   (tests/score_wide_cases.py FLOOR_Z)" % (worst32, floor_z), ""]
    for k, (en, wz, wy) in table.items():
        bad = [n for n, (eh, et), fl in (("nll", en, SC.FLOOR), ("z", wz, floor_z), ("y", wy, floor_z)) if eh > max(SC.RATIO * et, fl)]
        if bad:
            lines.append("ABOVE THE BAR: %s %s" % (k, " ".join(bad)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if args.wide:
    wide()
    sys.exit(0)
lines = ["WaveNet scoring: per-sample error against the float64 torch restatement on the whole utterance (scripts/score_parity.py)",
         "library %s on %s" % (_lib.lib().twv_version().decode(), torch.cuda.get_device_name(0)),
         "e = max|nll - nll64| / max|nll64| per utterance; bar: e_hip <= max(%g * e_t32, %g)" % (SC.RATIO, SC.FLOOR), "",
         "%-18s %6s %4s %9s %10s %10s %7s  %s" % ("case", "window", "utt", "positions", "e_hip", "e_t32", "ratio", "route")]
worst_quiet = ("", 0.0)            # the worst e_hip among utterances the float32 model gets right to 1e-7
for cid in SC.IDS:
    c = SC.case(cid)
    n64, n32 = SC.reference(cid)
    for wf in c.windows:
        sc = c.scorer(wf)
        r = sc.route()
        got = [v.cpu().numpy() for v in sc.score(c.audios, c.mels, c.gcs)]
        for i, g in enumerate(got):
            e_hip, e_t32 = SC.errors(g, n64[i], n32[i])
            ok = e_hip <= max(SC.RATIO * e_t32, SC.FLOOR)
            lines.append("%-18s %6d %4d %9d %10.3e %10.3e %7.2f  lc=%s head=%s loss=%s%s" % (cid, wf, i, g.size, e_hip, e_t32, e_hip / max(e_t32, 1e-30),
                                                                                             r["lc"], r["head"], r["loss"], "" if ok else "   ABOVE THE BAR"))
            if e_t32 < 1e-7 and e_hip > worst_quiet[1]:
                worst_quiet = ("%s window %d utterance %d" % (cid, wf, i), e_hip)
lines += ["", "worst e_hip where e_t32 < 1e-7: %.3e (%s)" % (worst_quiet[1], worst_quiet[0] or "no such utterance"), "",
          "%-18s %9s %15s %15s %15s %10s %10s" % ("case", "samples", "held-out loss", "float64 mean", "float32 mean", "|l-l64|", "|l32-l64|")]
for cid in SC.IDS:
    c = SC.case(cid)
    l64, l32 = SC.means(cid)
    loss, count = c.scorer().held_out_loss(c.audios, c.mels, c.gcs)
    lines.append("%-18s %9d %15.9f %15.9f %15.9f %10.2e %10.2e" % (cid, count, loss, l64, l32, abs(loss - l64), abs(l32 - l64)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
