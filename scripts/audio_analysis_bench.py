#!/usr/bin/env python
"""Times audio.spectrograms (framing kernel, hipFFT, fused linear + mel output kernel) against the plain PyTorch-ROCm composition of the
same function (torch.stft with the padded Hann window and reflect centring, abs, matmul with the dense mel basis, log10 / clamp), the
two alternating in one process on device-resident input, and states the bytes one pass must move.  Writes
profiles/audio_analysis_bench.txt.  Needs the GPU.  Sizes: B = 64 x 192 000 samples (8 s) and the training crop, B = 64 x 15 000."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3          # achievable HBM bandwidth of one MI355X, TB/s (the figure the byte floor is turned into time with)


def torch_composition(x, hp, basis_t, window):
    """utils/audio.py:61-75 in stock tensor operations -> (mel, linear), (B, frames, channels)"""
    import torch
    k = hp.preemphasis
    y = torch.cat([x[:, :1], x[:, 1:] - k * x[:, :-1]], dim=1)
    D = torch.stft(y, hp.fft_size, hop_length=hp.hop_size, win_length=hp.fft_size, window=window, center=True, pad_mode="reflect",
                   return_complex=True)
    mag = D.abs().transpose(1, 2)
    min_level = 10.0 ** (hp.min_level_db / 20.0)

    def norm(a):
        S = 20.0 * torch.log10(torch.clamp(a, min=min_level)) - hp.ref_level_db
        return torch.clamp((2 * hp.max_abs_value) * ((S - hp.min_level_db) / (-hp.min_level_db)) - hp.max_abs_value, -hp.max_abs_value, hp.max_abs_value)
    return norm(torch.matmul(mag, basis_t)), norm(mag)


def byte_floor(B, n, hp):
    rows = B * (1 + n // hp.hop_size)
    nbin = hp.fft_size // 2 + 1
    parts = {"wav read": B * n * 4, "frames written + read": 2 * rows * hp.fft_size * 4, "spectrum written + read": 2 * rows * nbin * 8,
             "linear written": rows * nbin * 4, "mel written": rows * hp.num_mels * 4}
    return parts, sum(parts.values())


def main(out=os.path.join(ROOT, "profiles", "audio_analysis_bench.txt"), calls=60):
    import numpy as np
    import torch
    import twvk_amd
    from twvk_amd import audio
    hp = twvk_amd.default_hparams()
    dev = torch.device("cuda:0")
    basis = audio.mel_basis(hp)
    basis_t = torch.from_numpy(basis.T.copy()).to(dev)
    lpad = (hp.fft_size - hp.win_size) // 2
    window = torch.zeros(hp.fft_size, device=dev)
    window[lpad:lpad + hp.win_size] = torch.hann_window(hp.win_size, periodic=True, device=dev)
    lines = ["audio.spectrograms vs the PyTorch-ROCm composition; default hparams; library %s on %s; torch %s"
             % (twvk_amd._lib.lib().twv_version().decode(), torch.cuda.get_device_name(0), torch.__version__),
             "median of %d calls each, alternating in one process, device-resident input, every call ends in a synchronise" % calls]
    ok = True
    for B, n in ((64, 192000), (64, 15000)):
        x = (torch.rand((B, n), device=dev) - 0.5) * 0.6
        for _ in range(3):                                        # warm this shape: plans, workspaces, allocator
            mel, lin = audio.spectrograms(x, hp); torch.cuda.synchronize()
            tm, tl = torch_composition(x, hp, basis_t, window); torch.cuda.synchronize()
        d_l, d_m = float((lin - tl).abs().max()), float((mel - tm).abs().max())
        del mel, lin, tm, tl
        t_hip, t_torch = [], []
        for _ in range(calls):
            t0 = time.perf_counter(); r = audio.spectrograms(x, hp); torch.cuda.synchronize(); t_hip.append(time.perf_counter() - t0)
            del r
            t0 = time.perf_counter(); r = torch_composition(x, hp, basis_t, window); torch.cuda.synchronize(); t_torch.append(time.perf_counter() - t0)
            del r
        a, b = float(np.median(t_hip)) * 1e3, float(np.median(t_torch)) * 1e3
        parts, total = byte_floor(B, n, hp)
        floor_ms = total / (HBM_TBS * 1e12) * 1e3
        lines.append("B = %d x %d samples (%d frames each):" % (B, n, 1 + n // hp.hop_size))
        lines.append("  hand-written path   median %.3f ms  (min %.3f, max %.3f)" % (a, min(t_hip) * 1e3, max(t_hip) * 1e3))
        lines.append("  torch composition   median %.3f ms  (min %.3f, max %.3f)" % (b, min(t_torch) * 1e3, max(t_torch) * 1e3))
        lines.append("  ratio torch / hand-written %.2f;  the two agree to %.2e (linear) %.2e (mel)" % (b / a, d_l, d_m))
        lines.append("  bytes one pass must move: %.3f GB (%s) = %.3f ms at %.1f TB/s; hand-written path at %.1f x that floor"
                     % (total / 1e9, ", ".join("%s %.0f MB" % (k, v / 1e6) for k, v in parts.items()), floor_ms, HBM_TBS, a / floor_ms))
        ok = ok and a <= b
    lines.append("hand-written median no larger than the torch composition's at both sizes: %s" % ok)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
