#!/usr/bin/env python
"""Per-sample error of WaveNet scoring against the float64 checker, for every case, window and utterance of tests/score_cases.py:
e = max|nll - nll64| / max|nll64| for the HIP path (e_hip) and for the float32 torch run of the same lines (e_t32), the ratio, and
the held-out loss beside the float64 and float32 means.  Writes --out (default profiles/wavenet_score_parity.txt).  Needs the GPU."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import score_cases as SC
import twvk_amd
from twvk_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavenet_score_parity.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
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
