#!/usr/bin/env python
"""The decoder gradients at the softmax attention types and loc_sen (twv_tacotron_decoder_grad_create_any) against the float64 autograd
checker, for every case of tests/tacotron_attention_grad_cases.py.

    python scripts/tacotron_attention_grad_parity.py --seeds [--case NAME] [--search]     # host only
        the three conditions of the case table in the float64 checker -- zero tensors, the worst e_t32, the largest alignment of each
        utterance -- at the table's (seed, sharpen); --search: also at the next seeds and other factors (how the table was chosen).
        Appends to --out.
    python scripts/tacotron_attention_grad_parity.py                                       # needs the GPU
        per tensor e = max|g - g64| / max|g64| of the HIP pass (e_hip) and of the float32 autograd run (e_t32), their ratio, and
        whether the floor of the bar was needed.  Appends to --out.

The T_in > 512 case is a Bahdanau type: loc_sen at (2, 530, (530, 301), 3) has e_t32 = 5.7e-4 on location_features_convolution/bias
(seed 201, unscaled), above condition 2's 1e-4, so the 8 x bar would say nothing there."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import tacotron_attention_grad_cases as K

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tacotron_attention_grad_parity.txt"))
ap.add_argument("--seeds", action="store_true")
ap.add_argument("--search", action="store_true")
ap.add_argument("--case", default=None)
args = ap.parse_args()
names = [args.case] if args.case else list(K.CASES)
lines = []

if args.seeds:
    lines += ["conditions of tests/tacotron_attention_grad_cases.py in the float64 checker (host only; memory and the initial states from the",
              "float64 encoder restatement): 1. no identically-zero gradient tensor, 2. worst e_t32 <= 1e-4, 3. the largest alignment of every",
              "utterance longer than three positions in [0.2, 0.98]", ""]
    for name in names:
        seed0, sharpen0 = K.CASES[name][-2:]
        trials = [(seed0, sharpen0)]
        if args.search:
            trials += [(seed0, f) for f in (1.0, 3.0, 6.0, 12.0, 24.0) if f != sharpen0] + [(seed0 + i, sharpen0) for i in (1, 2, 3)]
        for seed, f in trials:
            c = K.HostCase(name, seed=seed, sharpen=f)
            zero, worst, amax = c.conditions()
            line = "%-34s seed %4d sharpen %5.1f (%s): zero tensors %s, worst e_t32 %.2e (%s), largest alignment per utterance %s -> %s" % (
                name, seed, f, K.SHARPENED[c.at], zero or "none", worst[0], worst[1], " / ".join("%.3f" % a for a in amax),
                "hold" if K.conditions_hold(c, zero, worst, amax) else "DO NOT HOLD")
            print(line, flush=True)
            lines.append(line + ("   <- the table" if (seed, f) == (seed0, sharpen0) else ""))
    for name in ([] if args.case else sorted(K.WHOLE)):
        ok, fig = K.WholeCase(name).whole_conditions()
        line = "%-34s seed %4d sharpen %5.1f: %s -> %s" % (name, K.WHOLE[name][1], K.WHOLE[name][2], fig, "hold" if ok else "DO NOT HOLD")
        print(line, flush=True)
        lines.append(line)
else:
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    import test_tacotron_attention_grad_gpu as TG
    from train_cases import FLOOR, RATIO
    from twvk_amd import _lib
    lines += ["Tacotron decoder gradients at the softmax attention types and loc_sen (tg_forward_kernel<AK> / tg_backward_kernel<AK> + rocBLAS",
              "weight products) against the float64 autograd checker (the cases of tests/tacotron_attention_grad_cases.py)",
              "library %s on %s" % (_lib.lib().twv_version().decode(), torch.cuda.get_device_name(0)),
              "e = max|g - g64| / max|g64| per tensor; bar e_hip <= max(%g * e_t32, %g); 'floor' = e_hip > %g * e_t32" % (RATIO, FLOOR, RATIO), ""]
    summary = []
    for name in names:
        c = TG._case(name)
        mel64, g64, _ = c.checker("float64")
        _, g32, _ = c.checker("float32")
        got = c.hip()
        lines += ["case %s: N %d, T_in %d, lengths %s, %d steps, attention %s, layers %d, masks %s, seed %d, sharpen %g"
                  % (name, c.N, c.T, [int(v) for v in c.ln], c.steps, c.at, c.hp.dec_layer_num, c.masks is not None, c.seed, c.sharpen),
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
        summary.append("%-34s worst e_hip %.3e, mel %.3e, above the bar: %s" % (name, worst, e_mel, failed or "none"))
    lines += ["summary"] + ["  " + s for s in summary]
text = "\n".join(lines) + "\n\n"
with open(args.out, "a") as fh:
    fh.write(text)
if not args.seeds:
    print(text)
