#!/usr/bin/env python
"""Times audio.resample (one kernel: int16 -> float, channel average and the polyphase sum) against (a) the PyTorch-ROCm composition
of the same definition -- one strided conv1d with L output channels, one per phase, on the device -- and (b)
scipy.signal.resample_poly with the same taps on the CPU.  Kernel and composition alternate in one process on device-resident input,
every call ends in a synchronise; each figure is a median.  Writes profiles/resample_bench.txt.  Needs the GPU.
Cases: B = 64 x 8 s of 44.1 kHz stereo int16 -> 24 kHz (the layout of the reference's sample data), 48 kHz -> 24 kHz, 16 kHz -> 24 kHz
and 44.1 kHz -> 16 kHz (the pair whose tile takes 16 lanes per phase), mono float32."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_TBS = 6.3          # achievable HBM bandwidth of one MI355X, TB/s


def phase_filters(sr_in, sr_out):
    """the library's own table as conv1d weights (L, 1, M + taps): channel p of output r is y[p + L r], its window starts at
    x[r M - taps / 2]"""
    import numpy as np
    from twvk_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()
    _lib.check(lib.twv_resample_create(sr_in, sr_out, 1, 1, C.byref(h)))
    L, taps = lib.twv_resample_phases(h), lib.twv_resample_taps(h)
    tab = np.empty((L, taps), np.float32)
    _lib.check(lib.twv_resample_filter_host(h, tab.ctypes.data_as(C.c_void_p)))
    name = lib.twv_resample_kernel_name(h).decode()
    lib.twv_resample_destroy(h)
    M = sr_in // (sr_out // L)
    w = np.zeros((L, 1, M + taps), np.float32)
    for p in range(L):
        q0, row = divmod(p * M, L)
        w[p, 0, q0 + taps - np.arange(taps)] = tab[row]
    return w, L, M, taps, name


def torch_composition(x, w, L, M, taps, n_out):
    import torch
    if x.dtype == torch.int16:
        x = x.to(torch.float32) * (1.0 / 32768.0)
    if x.dim() == 3:
        x = x.mean(dim=2)
    rounds = -(-n_out // L)
    need = (rounds - 1) * M + M + taps                      # samples the last window ends at, counted from -taps / 2
    xp = torch.nn.functional.pad(x, (taps // 2, max(0, need - taps // 2 - x.shape[1])))
    y = torch.nn.functional.conv1d(xp[:, None, :], w, stride=M)             # (B, L, rounds)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :n_out]


def main(out=os.path.join(ROOT, "profiles", "resample_bench.txt"), calls=21, cpu_calls=5):
    import numpy as np
    import torch
    from scipy.signal import resample_poly
    import resample_ref as R
    import twvk_amd
    from twvk_amd import audio
    dev = torch.device("cuda:0")
    calls, cpu_calls = int(calls), int(cpu_calls)
    lines = ["audio.resample vs the PyTorch-ROCm composition (one strided conv1d, L output channels) vs scipy.signal.resample_poly on the CPU",
             "library %s on %s; torch %s" % (twvk_amd._lib.lib().twv_version().decode(), torch.cuda.get_device_name(0), torch.__version__),
             "kernel and composition: median of %d calls each, alternating in one process, device-resident input, every call ends in a synchronise; "
             "scipy: median of %d calls on float64 host arrays (%d CPUs visible, a shared host)" % (calls, cpu_calls, os.cpu_count() or 0)]
    B, seconds = 64, 8
    for sr_in, sr_out, stereo_int16 in ((44100, 24000, True), (48000, 24000, False), (16000, 24000, False), (44100, 16000, False)):
        n = sr_in * seconds
        g = torch.Generator(device="cpu").manual_seed(sr_in + sr_out)
        if stereo_int16:
            x = torch.randint(-20000, 20000, (B, n, 2), generator=g, dtype=torch.int16).to(dev)
        else:
            x = ((torch.rand((B, n), generator=g) - 0.5) * 1.2).to(dev)
        w_np, L, M, taps, name = phase_filters(sr_in, sr_out)
        w = torch.from_numpy(w_np).to(dev)
        n_out = R.out_samples(n, sr_in, sr_out)
        for _ in range(3):
            y, _ = audio.resample(x, sr_in, sr_out); torch.cuda.synchronize()
            yt = torch_composition(x, w, L, M, taps, n_out); torch.cuda.synchronize()
        agree, peak = float((y - yt).abs().max()), float(y.abs().max())
        del y, yt
        t_hip, t_torch = [], []
        for _ in range(calls):
            t0 = time.perf_counter(); r = audio.resample(x, sr_in, sr_out); torch.cuda.synchronize(); t_hip.append(time.perf_counter() - t0)
            del r
            t0 = time.perf_counter(); r = torch_composition(x, w, L, M, taps, n_out); torch.cuda.synchronize(); t_torch.append(time.perf_counter() - t0)
            del r
        xh = x.cpu().numpy()
        xh = (xh.astype(np.float64) / 32768.0).mean(axis=2) if stereo_int16 else xh.astype(np.float64)
        ptaps = R.poly_taps(sr_in, sr_out)
        t_cpu = []
        for i in range(cpu_calls + 1):
            t0 = time.perf_counter(); yc = resample_poly(xh, L, M, axis=1, window=ptaps); dt = time.perf_counter() - t0
            if i:
                t_cpu.append(dt)
        y, _ = audio.resample(x, sr_in, sr_out)
        d_cpu = float(np.abs(y.cpu().numpy() - yc).max())
        del y
        a, b, c = float(np.median(t_hip)) * 1e3, float(np.median(t_torch)) * 1e3, float(np.median(t_cpu)) * 1e3
        total = x.numel() * x.element_size() + B * n_out * 4
        macs = B * n_out * taps
        lines.append("B = %d x %d s, %d Hz %s -> %d Hz (L = %d, M = %d, %d taps; %s; %d -> %d samples):"
                     % (B, seconds, sr_in, "stereo int16" if stereo_int16 else "mono float32", sr_out, L, M, taps,
                        name, n, n_out))
        lines.append("  hand-written kernel  median %.3f ms  (min %.3f, max %.3f)   %.2f TFLOP/s of multiply-adds" % (a, min(t_hip) * 1e3, max(t_hip) * 1e3, 2 * macs / (a * 1e-3) / 1e12))
        lines.append("  torch composition    median %.3f ms  (min %.3f, max %.3f)" % (b, min(t_torch) * 1e3, max(t_torch) * 1e3))
        lines.append("  scipy resample_poly  median %.1f ms  (min %.1f, max %.1f)" % (c, min(t_cpu) * 1e3, max(t_cpu) * 1e3))
        lines.append("  ratios: torch / kernel %.2f, scipy / kernel %.0f;  kernel vs torch agree to %.2e, kernel vs scipy (float64) to %.2e, peak %.3f"
                     % (b / a, c / a, agree, d_cpu, peak))
        lines.append("  bytes one pass must move: %.1f MB = %.3f ms at %.1f TB/s; the kernel takes %.1f x that" % (total / 1e6, total / (HBM_TBS * 1e12) * 1e3, HBM_TBS, a / (total / (HBM_TBS * 1e12) * 1e3)))
        del x, w
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as fh:                              # after every case: a later one that fails keeps the earlier figures
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
