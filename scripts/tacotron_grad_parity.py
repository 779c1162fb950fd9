#!/usr/bin/env python
"""Per-tensor error of the Tacotron decoder gradients against the float64 autograd checker (tests/torch_tacotron_grad_ref.py), for every
case of tests/tacotron_grad_cases.py: e = max|g - g64| / max|g64| for the HIP pass (e_hip) and for the float32 autograd run of the same
lines (e_t32), their ratio, and whether the floor of the bar was needed.  Writes --out (default profiles/tacotron_decoder_grad_parity.txt).
Needs the GPU."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import test_tacotron_grad_gpu as TG        # the device side of a case (_case) and RTOL; the table itself is tests/tacotron_grad_cases.py
from tacotron_grad_cases import CASES
from train_cases import FLOOR, RATIO
from twvk_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tacotron_decoder_grad_parity.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"

lines = ["Tacotron decoder gradients (tg_forward_kernel / tg_backward_kernel + rocBLAS weight products) against the float64 autograd checker",
         "(scripts/tacotron_grad_parity.py; the cases of tests/tacotron_grad_cases.py)",
         "library %s on %s" % (_lib.lib().twv_version().decode(), torch.cuda.get_device_name(0)),
         "e = max|g - g64| / max|g64| per tensor; bar e_hip <= max(%g * e_t32, %g); 'floor' = e_hip > %g * e_t32 (the floor carried the tensor)" % (RATIO, FLOOR, RATIO), ""]
summary = []
for name in sorted(CASES):
    c = TG._case(name)
    mel64, g64, rec = c.checker("float64")
    _, g32, _ = c.checker("float32")
    got = c.hip()
    lines += ["case %s: N %d, T_in %d, lengths %s, %d steps, attention %s, layers %d, masks %s; cumprod margin %.3g, min(1 - p) %.3g, clamp engaged %s"
              % (name, c.N, c.T, [int(v) for v in c.ln], c.steps, c.at, c.hp.dec_layer_num, c.masks is not None, rec["cumprod_margin"], rec["min_one_minus_p"],
                 rec["clamp_engaged"]),
              "  %-98s %10s %10s %8s" % ("tensor", "e_hip", "e_t32", "ratio")]
    worst, failed = 0.0, []
    for k in g64:
        scale = max(float(np.abs(g64[k]).max()), 1e-30)
        e_hip = float(np.abs(got[k].astype(np.float64) - g64[k]).max()) / scale
        e_t32 = float(np.abs(g32[k].astype(np.float64) - g64[k]).max()) / scale
        ok = e_hip <= max(RATIO * e_t32, FLOOR)
        failed += [] if ok else [k]
        worst = max(worst, e_hip)
        lines.append("  %-98s %10.3e %10.3e %8.2f%s%s" % (k, e_hip, e_t32, e_hip / max(e_t32, 1e-30), "  floor" if e_hip > RATIO * e_t32 else "",
                                                          "" if ok else "  ABOVE THE BAR"))
    e_mel = float(np.abs(got["mel"] - mel64).max()) / float(np.abs(mel64).max())
    lines += ["  recorded forward: mel e_hip %.3e (bar %g)" % (e_mel, TG.RTOL), ""]
    summary.append("%-20s worst e_hip %.3e, mel %.3e, above the bar: %s" % (name, worst, e_mel, failed or "none"))
lines += ["summary"] + ["  " + s for s in summary]
text = "\n".join(lines) + "\n"
with open(args.out, "w") as fh:
    fh.write(text)
print(text)
