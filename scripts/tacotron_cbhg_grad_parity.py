#!/usr/bin/env python
"""Per-tensor error of the Tacotron encoder and post-net gradients against the float64 autograd checker
(tests/torch_tacotron_cbhg_grad_ref.py), for every case of tests/tacotron_cbhg_grad_cases.py on both sides: e = max|g - g64| / max|g64| for
the HIP pass (e_hip) and for the float32 autograd run of the same lines (e_t32), their ratio, and whether the floor of the bar was needed;
the margins of each case.  Writes --out (default profiles/tacotron_cbhg_grad_parity.txt).  Needs the GPU.

--seeds NAME: host only -- the margins of case NAME for the ten seeds from its own on (how the table's seeds were chosen)."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import tacotron_cbhg_grad_cases as K
from train_cases import FLOOR, RATIO
from twvk_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tacotron_cbhg_grad_parity.txt"))
ap.add_argument("--seeds", default=None)
args = ap.parse_args()
if args.seeds:
    base = K.CASES[args.seeds][-1]
    for s in range(base, base + 10):
        print("%s seed %d: same branches %s, relu margin %.3e, pool gap %.3e" % ((args.seeds, s) + K.HostCase(args.seeds, seed=s).margins()))
    sys.exit(0)
assert torch.cuda.is_available(), "a measurement needs the GPU"
import test_tacotron_cbhg_grad_gpu as TG

lines = ["Tacotron encoder / post-net gradients (cg_gru_forward_kernel / cg_gru_backward_kernel, the row and pointwise kernels, rocBLAS weight",
         "products) against the float64 autograd checker (scripts/tacotron_cbhg_grad_parity.py; the cases of tests/tacotron_cbhg_grad_cases.py)",
         "library %s on %s" % (_lib.lib().twv_version().decode(), torch.cuda.get_device_name(0)),
         "e = max|g - g64| / max|g64| per tensor; bar e_hip <= max(%g * e_t32, %g); 'floor' = e_hip > %g * e_t32 (the floor carried the tensor)" % (RATIO, FLOOR, RATIO), ""]
summary = []
for name in sorted(K.CASES):
    c = TG._case(name)
    h = c.h
    for side, checker, hip, fwd in (("encoder", h.encoder_checker, c.encoder_hip, "memory"), ("post net", h.postnet_checker, c.postnet_hip, "linear")):
        o64, g64, rec = checker("float64")
        _, g32, _ = checker("float32")
        got = hip()
        lines += ["case %s, %s: N %d, T %d, lengths %s, speakers %d, masks %s; relu margin %.3g, pool gap %.3g"
                  % (name, side, h.N, h.T if side == "encoder" else h.TO, [int(v) for v in h.ln] if side == "encoder" else "-", h.speakers,
                     h.masks is not None and side == "encoder", rec["relu_margin"], rec["pool_gap"]),
                  "  %-78s %10s %10s %8s" % ("tensor", "e_hip", "e_t32", "ratio")]
        worst, ratio, failed, floor = 0.0, 0.0, [], []
        for k in g64:
            scale = max(float(np.abs(g64[k]).max()), 1e-30)
            e_hip = float(np.abs(got[k].astype(np.float64) - g64[k]).max()) / scale
            e_t32 = float(np.abs(g32[k].astype(np.float64) - g64[k]).max()) / scale
            ok = e_hip <= max(RATIO * e_t32, FLOOR)
            failed += [] if ok else [k]
            floor += [k] if e_hip > RATIO * e_t32 else []
            worst, ratio = max(worst, e_hip), max(ratio, e_hip / max(e_t32, 1e-30))
            lines.append("  %-78s %10.3e %10.3e %8.2f%s%s" % (k, e_hip, e_t32, e_hip / max(e_t32, 1e-30), "  floor" if e_hip > RATIO * e_t32 else "",
                                                              "" if ok else "  ABOVE THE BAR"))
        e_fwd = float(np.abs(got[fwd] - o64).max()) / float(np.abs(o64).max())
        lines += ["  recorded forward: %s e_hip %.3e (bar %g)" % (fwd, e_fwd, TG.RTOL), ""]
        summary.append("%-22s %-8s worst e_hip %.3e, worst ratio %5.2f, %s %.3e, needed the floor: %s, above the bar: %s"
                       % (name, side, worst, ratio, fwd, e_fwd, floor or "none", failed or "none"))
lines += ["summary"] + ["  " + s for s in summary]
text = "\n".join(lines) + "\n"
with open(args.out, "w") as fh:
    fh.write(text)
print(text)
