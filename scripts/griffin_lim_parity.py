#!/usr/bin/env python
"""Records the parity measurement of the Griffin-Lim tests (tests/test_audio_gpu.py: every geometry, pre-emphasis, batch, basis and
the grid-stride regime -- device vs float64 checker beside the float32 run of the checker and the bar derived from it) in
profiles/griffin_lim_parity.txt.  Needs the GPU.

    python scripts/griffin_lim_parity.py [out.txt [timing.txt]]      # timing.txt: the A/B record to keep below the parity rows
    python scripts/griffin_lim_parity.py --ragged [out.txt]          # APPENDS the rows of tests/test_griffin_lim_ragged_gpu.py (utterances of
                                                                     # unequal lengths in one call), same columns, and whether each ragged
                                                                     # utterance is bit-equal to its B = 1 call
    python scripts/griffin_lim_parity.py --time [reps]               # one number: ms of inv_linear_spectrogram at B = 32 x 1000 frames
                                                                     # x 60 iterations (median of reps), for scripts/ab_two_builds.sh
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_default(reps=7, B=32, T=1000, iters=60):
    """handle, plans and workspace made once and warmed up; each timed call is bracketed by device events"""
    import ctypes as C
    import numpy as np
    import torch
    import twvk_amd
    from twvk_amd import _lib
    from twvk_amd.audio import _ptr
    hp = twvk_amd.default_hparams()
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.twv_griffin_lim_create(hp.fft_size, hp.hop_size, hp.win_size, T, B, C.byref(h)))
    g = torch.Generator(device="cuda:0").manual_seed(0)
    lin = (torch.rand((B, T, hp.num_freq), device="cuda:0", generator=g) * 9.0 - 4.5).contiguous()
    u = torch.rand((B, T, hp.num_freq), device="cuda:0", generator=g).contiguous()
    ws = torch.empty(L.twv_griffin_lim_workspace_bytes(h) // 4 + 64, dtype=torch.float32, device="cuda:0")
    out = torch.empty((B, L.twv_griffin_lim_samples(h)), dtype=torch.float32, device="cuda:0")

    def call():
        _lib.check(L.twv_inv_linear_spectrogram(h, _ptr(lin), _ptr(u), iters, hp.power, hp.ref_level_db, hp.max_abs_value, hp.min_level_db,
                                                hp.preemphasis, _ptr(ws), _ptr(out), None))
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    L.twv_griffin_lim_destroy(h)
    assert bool(torch.isfinite(out).all())
    return float(np.median(ms)), ms


def main(out=os.path.join(ROOT, "profiles", "griffin_lim_parity.txt"), timing=None):
    import torch
    import twvk_amd
    import griffin_lim_cases as G
    from test_audio_gpu import parity_report
    lines = ["spectrogram -> waveform parity; library %s on %s" % (twvk_amd._lib.lib().twv_version().decode(), torch.cuda.get_device_name(0)),
             "e = max|. - float64 checker| / peak(float64 checker) per utterance; e_f32: the checker's lines run in float32 / complex64",
             "bar = max(%g x e_f32, %g); 'kernel alone' rows: the de-emphasis against the float64 recurrence on the device's own k = 0 output"
             % (G.MARGIN, G.FLOOR)]
    rows = parity_report(log=lines.append)
    lines.append("%d rows, worst e_gpu / e_f32 = %.2f, worst e_gpu / bar = %.3f, all within the bar: %s"
                 % (len(rows), max(r[2] / r[3] for r in rows if r[3]), max(r[2] / r[4] for r in rows), all(r[2] <= r[4] for r in rows)))
    if timing:
        lines.append("")
        lines += open(timing).read().rstrip("\n").split("\n")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def ragged(out=os.path.join(ROOT, "profiles", "griffin_lim_parity.txt")):
    import torch
    import twvk_amd
    from test_griffin_lim_ragged_gpu import ragged_parity_report
    lines = ["", "Utterances of unequal lengths in one call (twv_griffin_lim_create_ragged; tests/griffin_lim_ragged_cases.py); library %s on %s"
             % (twvk_amd._lib.lib().twv_version().decode(), torch.cuda.get_device_name(0)),
             "same columns; the float64 checker runs on each utterance alone, at its own length"]
    rows, equal = ragged_parity_report(log=lines.append)
    lines.append("%d rows, worst e_gpu / e_f32 = %.2f, worst e_gpu / bar = %.3f, all within the bar: %s"
                 % (len(rows), max(r[2] / r[3] for r in rows if r[3]), max(r[2] / r[4] for r in rows), all(r[2] <= r[4] for r in rows)))
    with open(out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--ragged":
        ragged(*sys.argv[2:3])
    elif len(sys.argv) > 1 and sys.argv[1] == "--time":
        med, ms = time_default(*[int(a) for a in sys.argv[2:3]])
        print("%.3f" % med)
        sys.stderr.write("runs (ms): %s\n" % " ".join("%.3f" % m for m in ms))
    else:
        main(*sys.argv[1:])
