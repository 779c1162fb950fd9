#!/usr/bin/env python
"""Times Griffin-Lim for utterances of unequal lengths: one ragged call against the per-utterance loop that Synthesizer.synthesize runs
by default, and the ragged kernels against the uniform ones at equal lengths.  Needs the GPU.

    python scripts/griffin_lim_ragged_bench.py [out.txt [reps]]      # default profiles/griffin_lim_ragged_bench.txt, 7 repetitions

Workload: default geometry (n_fft 2048, win 1200, hop 300), 60 iterations, k = 0.97, 32 utterances of seeded lengths in 89 ... 640 frames.
  user level   (a) one audio.inv_linear_spectrogram_list call; (b) audio.inv_linear_spectrogram(lin[None]) per utterance, as
               synthesizer.plot_graph_and_save_audio does.  Handle, hipFFT plans, workspace and the host-to-device copies are inside
               every timed window, as a user pays them; the uniforms are given (host float32), so no random draw is timed.
  warm, C ABI  the same work on handles, plans, workspaces and device inputs made before: (a) one call on one ragged handle, (b) one call
               on each of 32 uniform B = 1 handles.
  equal length the ragged handle at B = 32 x 1000 frames against the uniform handle at the same shape, warm, C ABI.
(a) and (b) alternate; every timed window ends with a device synchronise (host clock around it); medians and spreads (max - min) of
`reps` repetitions after a warm-up of every shape."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERS, N_UTT, LO, HI = 60, 32, 89, 640


def _timed(fn, torch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _alternate(a, b, reps, torch):
    ta, tb = [], []
    for _ in range(reps):
        ta.append(_timed(a, torch)); tb.append(_timed(b, torch))
    return ta, tb


def _line(name, ms):
    import numpy as np
    return "%-58s median %9.3f ms  spread %8.3f ms  runs %s" % (name, float(np.median(ms)), max(ms) - min(ms), " ".join("%.3f" % m for m in ms))


class _Warm(object):
    """a handle of either kind with its workspace, device inputs and output: call() is one twv_inv_linear_spectrogram"""

    def __init__(self, L, hp, frames, ragged, torch, gen):
        from twvk_amd import _lib
        import numpy as np
        self.L, self.hp, self.h = L, hp, C.c_void_p()
        if ragged:
            arr = np.asarray(frames, np.int32)
            _lib.check(L.twv_griffin_lim_create_ragged(hp.fft_size, hp.hop_size, hp.win_size, arr.ctypes.data_as(C.c_void_p), len(arr), C.byref(self.h)))
        else:
            B, T = frames
            _lib.check(L.twv_griffin_lim_create(hp.fft_size, hp.hop_size, hp.win_size, T, B, C.byref(self.h)))
        tf, ts = L.twv_griffin_lim_total_frames(self.h), L.twv_griffin_lim_total_samples(self.h)
        self.lin = (torch.rand((tf, hp.num_freq), device="cuda:0", generator=gen) * 9.0 - 4.5).contiguous()
        self.u = torch.rand((tf, hp.num_freq), device="cuda:0", generator=gen).contiguous()
        self.ws = torch.empty(L.twv_griffin_lim_workspace_bytes(self.h) // 4 + 64, dtype=torch.float32, device="cuda:0")
        self.out = torch.empty(ts, dtype=torch.float32, device="cuda:0")

    def call(self):
        from twvk_amd import _lib
        from twvk_amd.audio import _ptr
        hp = self.hp
        _lib.check(self.L.twv_inv_linear_spectrogram(self.h, _ptr(self.lin), _ptr(self.u), ITERS, hp.power, hp.ref_level_db, hp.max_abs_value,
                                                     hp.min_level_db, hp.preemphasis, _ptr(self.ws), _ptr(self.out), None))

    def destroy(self):
        self.L.twv_griffin_lim_destroy(self.h)


def main(out=os.path.join(ROOT, "profiles", "griffin_lim_ragged_bench.txt"), reps=7):
    import numpy as np
    import torch
    import twvk_amd
    from twvk_amd import _lib
    from twvk_amd.audio import inv_linear_spectrogram, inv_linear_spectrogram_list
    reps = int(reps)
    hp = twvk_amd.default_hparams()
    hp.griffin_lim_iters = ITERS
    L = _lib.lib()
    rng = np.random.RandomState(0)
    Ts = [int(t) for t in rng.randint(LO, HI + 1, N_UTT)]
    lins = [rng.uniform(-4.5, 4.5, (T, hp.num_freq)).astype(np.float32) for T in Ts]
    us = [rng.rand(T, hp.num_freq).astype(np.float32) for T in Ts]
    lines = ["Griffin-Lim, utterances of unequal lengths; library %s on %s" % (L.twv_version().decode(), torch.cuda.get_device_name(0)),
             "default geometry, %d iterations, k = %g; %d utterances, frames %s (total %d)" % (ITERS, hp.preemphasis, N_UTT, Ts, sum(Ts)),
             "host clock, a device synchronise inside every timed window; (a) and (b) alternate; %d repetitions after a warm-up of every shape" % reps,
             ""]

    def user_list():
        return inv_linear_spectrogram_list(lins, hp, uniforms=us)

    def user_loop():
        return [inv_linear_spectrogram(lin[None], hp, uniforms=u[None])[0] for lin, u in zip(lins, us)]
    a, b = user_list(), user_loop()                          # the warm-up of every shape, and a look at the results
    worst = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b))
    lines.append("user level: handle, plans, workspace and host-to-device copies inside the window")
    lines.append("largest |list - loop| / peak over the utterances: %.3e; bit-equal utterances: %d of %d"
                 % (worst, sum(bool(torch.equal(x, y)) for x, y in zip(a, b)), N_UTT))
    del a, b
    ta, tb = _alternate(user_list, user_loop, reps, torch)
    lines += [_line("(a) one inv_linear_spectrogram_list call", ta), _line("(b) inv_linear_spectrogram per utterance (%d calls)" % N_UTT, tb), ""]

    gen = torch.Generator(device="cuda:0").manual_seed(0)
    rag = _Warm(L, hp, Ts, True, torch, gen)
    singles = [_Warm(L, hp, (1, T), False, torch, gen) for T in Ts]

    def warm_loop():
        for s in singles:
            s.call()
    for _ in range(2):
        rag.call(); warm_loop()
    ta, tb = _alternate(rag.call, warm_loop, reps, torch)
    lines.append("warm, C ABI: handles, plans, workspaces and device inputs made before")
    lines += [_line("(a) one call on the ragged handle", ta), _line("(b) one call on each of %d uniform B = 1 handles" % N_UTT, tb), ""]
    rag.destroy()
    for s in singles:
        s.destroy()
    del rag, singles
    torch.cuda.empty_cache()

    B, T = 32, 1000
    uni, req = _Warm(L, hp, (B, T), False, torch, gen), _Warm(L, hp, [T] * B, True, torch, gen)
    req.lin.copy_(uni.lin); req.u.copy_(uni.u)
    for _ in range(2):
        uni.call(); req.call()
    tu, tr = _alternate(uni.call, req.call, reps, torch)
    torch.cuda.synchronize()
    lines.append("equal lengths, B = %d x %d frames, warm, C ABI (the uniform path's record: 54.8 ms, run-to-run spread 0.34 ms)" % (B, T))
    lines += [_line("uniform handle (twv_griffin_lim_create)", tu), _line("ragged handle, equal lengths", tr)]
    lines.append("ragged - uniform = %+.3f ms (medians); outputs bit-equal: %s"
                 % (float(np.median(tr) - np.median(tu)), bool(torch.equal(uni.out, req.out))))
    uni.destroy(); req.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(*sys.argv[1:3])
