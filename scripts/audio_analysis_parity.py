#!/usr/bin/env python
"""Records the parity measurement of tests/test_audio_analysis_gpu.py (the ragged batch of three utterances: device vs float64
checker, beside the float32 run of the checker and the bar derived from it) in profiles/audio_analysis_parity.txt.  Needs the GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out=os.path.join(ROOT, "profiles", "audio_analysis_parity.txt")):
    import torch
    import twvk_amd
    from test_audio_analysis_gpu import parity_report
    lines = ["waveform -> spectrogram parity, default hparams; library %s on %s" % (twvk_amd._lib.lib().twv_version().decode(), torch.cuda.get_device_name(0)),
             "bar = max(8 x max|float32 checker - float64 checker|, 1e-5), normalised units ([-4, 4])"]
    rows = parity_report(log=lines.append)
    lines.append("all within the bar: %s" % all(r[4] <= r[6] for r in rows))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(*sys.argv[1:])
