#!/usr/bin/env python
"""Records the parity measurement of tests/test_resample_gpu.py (thirteen rate pairs, one for every route of the kernel, each named
with its route -- instantiation, chunks, lanes that are not live, LDS bytes --, a ragged batch of five utterances each: device vs
float64 checker, beside the float32 run of the checker and the bar derived from it) in profiles/resample_parity.txt.  Needs the GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out=os.path.join(ROOT, "profiles", "resample_parity.txt")):
    import torch
    import twvk_amd
    from test_resample_gpu import parity_report
    lines = ["resampling parity (twv_resample vs tests/resample_ref.py); library %s on %s" % (twvk_amd._lib.lib().twv_version().decode(), torch.cuda.get_device_name(0)),
             "bar = max(8 x max|float32 checker - float64 checker|, 5e-6 x peak); seeded uniform noise in [-1, 1)"]
    rows = parity_report(log=lines.append)
    lines.append("largest max|gpu - f64| / peak: %.3e;  largest max|f32 checker - f64| / peak: %.3e" % (max(r[5] / r[8] for r in rows), max(r[6] / r[8] for r in rows)))
    lines.append("all within the bar: %s" % all(r[5] <= r[7] for r in rows))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(*sys.argv[1:])
