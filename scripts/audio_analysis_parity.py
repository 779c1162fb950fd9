#!/usr/bin/env python
"""Records the parity measurements of tests/test_audio_analysis_gpu.py (default hparams, the ragged batch of three utterances: device
vs float64 checker, beside the float32 run of the checker and the bar derived from it) and of
tests/test_audio_analysis_geometry_gpu.py (one line per row of tests/audio_analysis_cases.py's geometry table, utterance and output,
in the dB and the amplitude measure) in profiles/audio_analysis_parity.txt.  Needs the GPU."""
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
    from test_audio_analysis_geometry_gpu import parity_report as geometry_report
    lines += ["", "geometry table (tests/audio_analysis_cases.py), the row's own float32 basis on both sides; per (row, utterance, output):",
              "dB: max|. - f64| in normalised units, bar = max(8 x f32, 1e-5);  amplitude: e = max|a(.) - a(f64)| / max a(f64), bar = max(8 x e_f32, 1e-6)"]
    rows = geometry_report(log=lines.append)
    lines.append("all within both bars: %s;  largest e / e_f32: %.2f" % (all(r[3] <= r[5] and r[6] <= r[8] for r in rows), max(r[6] / r[7] for r in rows)))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(*sys.argv[1:])
