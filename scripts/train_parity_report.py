"""Training-step parity in numbers: for every geometry of the shared case table (tests/train_cases.py: the
geometries of tests/test_train_gpu.py, and the path cases of tests/test_train_paths_gpu.py with the route each one takes) the HIP
gradients and the float32 torch model's gradients against the float64 torch model, per tensor: e = max|g - g64| / max|g64|.  Prints,
per case, the worst e_hip, the worst e_t32, the worst ratio e_hip / max(e_t32, 1e-7) and the tensors they occur in -- the data behind
the bars the tests assert; with --paths only the path cases, followed by every tensor's e_hip, e_t32 and ratio; with --wide the cases
of tests/train_wide_cases.py at widths 64 and 128, each followed by its width-32 twin (the same model and data at width 32, through the
width-32 kernels), and the line `floor_g` that fixes the wide tests' gradient floor.  Run on the GPU box:
    python scripts/train_parity_report.py > profiles/r05_train_parity_report.txt
    python scripts/train_parity_report.py --paths > profiles/train_paths_parity_report.txt
    python scripts/train_parity_report.py --wide > profiles/wavenet_train_wide_parity.txt"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch_train_ref as R                      # noqa: E402
import train_cases as TC                         # noqa: E402

PATHS = "--paths" in sys.argv[1:]
CASES = [(name, kw, False) for name, kw in TC.DEFAULT_CASES] + [(name, kw, True) for name, kw in TC.BIG_CASES]
if PATHS:
    CASES = [(name, kw, False) for name, kw, _ in TC.PATH_CASES]
FLOOR = 1e-7          # below this a float32 tensor's own error says nothing (one ulp of its largest element)


def wide_report():
    import train_wide_cases as TW

    def figures(cid, width):
        tensors, cfg, audio, lc, gc, q = TW.data(cid, width)
        tr = TW.trainer(cid, width)
        loss = float(tr.loss_and_gradients(audio, lc, gc).item())
        got = tr.gradients()
        l64, g64, l32, g32 = TW.reference(cid, width)
        rows = []
        for k in g64:
            scale = max(float(np.abs(g64[k]).max()), 1e-30)
            rows.append((k, float(np.abs(got[k] - g64[k]).max()) / scale, float(np.abs(g32[k] - g64[k]).max()) / scale))
        return tr.route(), loss, l64, l32, rows

    print("%-30s %5s %10s %10s %8s   %s" % ("case", "width", "e_hip", "e_t32", "ratio", "worst tensor (by e_hip); tensors over the bar max(8 e_t32, 5e-6)"))
    worst_wide, worst_twin, worst_exact, need = 0.0, 0.0, 0.0, 0.0
    for cid, W, kw, _ in TW.CASES:
        for width in (W, 32):
            route, loss, l64, l32, rows = figures(cid, width)
            wh = max(rows, key=lambda r: r[1]); wt = max(rows, key=lambda r: r[2]); wr = max(rows, key=lambda r: r[1] / max(r[2], FLOOR))
            over = [r for r in rows if r[1] > max(TC.RATIO * r[2], TC.FLOOR)]
            print("%-30s %5d %10.3g %10.3g %8.2f   %s; %d over" % (cid if width == W else "  twin", width, wh[1], wt[2], wr[1] / max(wr[2], FLOOR),
                                                                  wh[0].replace("wavenet/", ""), len(over)))
            print("%-30s       loss hip %.7f  f32 %.7f  f64 %.7f   |hip-f64| %.2e  |f32-f64| %.2e   %s" % ("", loss, l32, l64, abs(loss - l64), abs(l32 - l64),
                                                                                                   " ".join("%s=%s" % kv for kv in route.items() if kv[0] != "carve_floats")))
            exact = max([r[1] for r in rows if r[2] < FLOOR] or [0.0])      # where the float32 model is itself exact
            if width == W:
                worst_wide, worst_exact = max(worst_wide, wh[1]), max(worst_exact, exact)
                need = max([need] + [r[1] for r in over if r[2] < FLOOR])
            else:
                worst_twin = max(worst_twin, wh[1])
            torch.cuda.empty_cache()
    floor_g = TC.FLOOR if need <= TC.FLOOR else min(need, 2 * worst_twin)
    print("floor_g %.3g   (project FLOOR %.3g; worst wide e_hip %.3g, worst wide e_hip where e_t32 < 1e-7: %.3g; worst width-32 twin e_hip %.3g, "
          "limit 2 x that = %.3g; a wide tensor over the bar where the float32 model is exact needs %.3g)"
          % (floor_g, TC.FLOOR, worst_wide, worst_exact, worst_twin, 2 * worst_twin, need))


if "--wide" in sys.argv[1:]:
    wide_report()
    sys.exit(0)

print("%-26s %10s %10s %8s   %s" % ("case", "e_hip", "e_t32", "ratio", "worst tensor (by e_hip) | (by ratio)"))
for name, kw, big in CASES:
    tr, tensors, cfg, audio, lc, gc, quantized = TC._case6(**kw)
    loss = float(tr.loss_and_gradients(audio, lc, gc).item())
    got = tr.gradients()
    extra = dict(device="cuda:0", matmul_form=True) if big else {}
    extra["quantized"] = quantized
    l64, g64 = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float64, **extra)
    torch.cuda.empty_cache()
    l32, g32 = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float32, **extra)
    torch.cuda.empty_cache()
    rows = []
    for k in g64:
        scale = max(float(np.abs(g64[k]).max()), 1e-30)
        e_hip = float(np.abs(got[k] - g64[k]).max()) / scale
        e_t32 = float(np.abs(g32[k] - g64[k]).max()) / scale
        rows.append((k, e_hip, e_t32, e_hip / max(e_t32, FLOOR), scale))
    wh = max(rows, key=lambda r: r[1]); wr = max(rows, key=lambda r: r[3]); wt = max(rows, key=lambda r: r[2])
    print("%-26s %10.3g %10.3g %8.2f   %s | %s (e_hip %.3g, e_t32 %.3g)" % (name, wh[1], wt[2], wr[3], wh[0].replace("wavenet/", ""), wr[0].replace("wavenet/", ""), wr[1], wr[2]))
    print("%-26s loss hip %.7f  f32 %.7f  f64 %.7f   |hip-f64| %.2e  |f32-f64| %.2e" % ("", loss, l32, l64, abs(loss - l64), abs(l32 - l64)))
    # distribution: how many tensors above a few thresholds
    for th in (1e-3, 3e-4, 1e-4, 3e-5):
        n = sum(1 for r in rows if r[1] > th)
        print("%-26s   tensors with e_hip > %.0e: %d of %d" % ("", th, n, len(rows)), ("(" + ", ".join(r[0].split("/")[-3] + "/" + r[0].split("/")[-2] for r in rows if r[1] > th)[:160] + ")") if 0 < n <= 6 else "")
    if PATHS:
        print("%-26s route: %s" % ("", " ".join("%s=%s" % kv for kv in tr.route().items())))
        for k, e_hip, e_t32, ratio, scale in rows:
            print("%-26s   %-64s e_hip %9.3g  e_t32 %9.3g  ratio %8.2f  max|g64| %9.3g" % ("", k.replace("wavenet/", ""), e_hip, e_t32, ratio, scale))
    del tr
    torch.cuda.empty_cache()
