#!/usr/bin/env python
"""Times of the Tacotron encoder / post-net gradient passes (Tacotron.encoder_grad, postnet_grad) and of the whole loss_gradients chain at
the default geometry: B = 8 and B = 32, 101 tokens, 200 decoder steps (T_out = 1000), the weights of scripts/tacotron_bench.py.  Per batch
and side: the four phases of the run from its own events (recording forward, the GRUs' backward through time, the row-wise backward =
pointwise kernels + dx products, the weight-gradient products), the BPTT time per GRU step, and -- the yardstick -- the PyTorch-ROCm float32
autograd pass (forward + backward) of the same graph on the same device.  Medians of --passes runs.  Writes --out (default
profiles/tacotron_cbhg_grad_bench.txt).  Needs the GPU."""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np, torch
import torch.nn.functional as F
import twvk_amd
from twvk_amd import _lib
from twvk_amd.tacotron import Tacotron
from tacotron_targets_bench import random_tensors

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tacotron_cbhg_grad_bench.txt"))
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--torch-passes", type=int, default=2)
ap.add_argument("--batches", default="8,32")
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
T, STEPS = 101, 200


def torch_cbhg(w, x, lengths, scope, bank, depth, bh=None, init=None):
    """float32 autograd on the device: modules.py:25-74 in inference mode (the graph the hand-written pass differentiates)"""
    def conv(x, p, relu):
        k = w[p + "/conv1d/kernel"]
        kw = k.shape[0]
        y = F.conv1d(F.pad(x.transpose(1, 2), ((kw - 1) // 2, (kw - 1) - (kw - 1) // 2)), k.permute(2, 1, 0)).transpose(1, 2) + w[p + "/conv1d/bias"]
        y = torch.relu(y) if relu else y
        g, b, m, v = w[p + "/batch_normalization"]
        return (y - m) / torch.sqrt(v + 1e-3) * g + b

    def gru(x, h, p):
        n = h.shape[1]
        g = torch.sigmoid(torch.cat([x, h], 1) @ w[p + "/gates/kernel"] + w[p + "/gates/bias"])
        r, u = g[:, :n], g[:, n:]
        c = torch.tanh(torch.cat([x, r * h], 1) @ w[p + "/candidate/kernel"] + w[p + "/candidate/bias"])
        return u * h + (1.0 - u) * c
    N, Tn, _ = x.shape
    y = torch.cat([conv(x, "%s/conv_bank/conv1d_%d" % (scope, k), True) for k in range(1, bank + 1)], 2)
    later = torch.cat([y[:, 1:], torch.full_like(y[:, :1], -float("inf"))], 1)
    y = torch.where(later > y, later, y)
    y = conv(conv(y, scope + "/proj_1", True), scope + "/proj_2", False) + x
    if bh is not None:
        y = y + bh[:, None, :]
    if scope + "/dense/kernel" in w:
        y = y @ w[scope + "/dense/kernel"] + w[scope + "/dense/bias"]
    for i in range(depth):
        p = "%s/highway_%d" % (scope, i + 1)
        Hh = torch.relu(y @ w[p + "/H/kernel"] + w[p + "/H/bias"]); Tg = torch.sigmoid(y @ w[p + "/T/kernel"] + w[p + "/T/bias"])
        y = Hh * Tg + y * (1.0 - Tg)
    outs = []
    for d, order in (("fw", range(Tn)), ("bw", range(Tn - 1, -1, -1))):
        h = torch.zeros(N, 128, device=x.device) if init is None else (init[:, :128] if d == "fw" else init[:, 128:])
        o = [None] * Tn
        for t in order:
            live = (t < lengths)[:, None]
            hn = gru(y[:, t], h, "%s/bidirectional_rnn/%s/gru_cell" % (scope, d))
            h = torch.where(live, hn, h); o[t] = torch.where(live, hn, torch.zeros_like(hn))
        outs.append(torch.stack(o, 1))
    return torch.cat(outs, 2)


def med(fn, passes, warm=1):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(passes):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


hp = twvk_amd.default_hparams()
m = Tacotron(hp, num_speakers=2)
tensors = random_tensors(m.specs)
m.load_weights(tensors)
L = _lib.lib()
lines = ["Tacotron encoder / post-net gradient passes (Tacotron.encoder_grad / postnet_grad / loss_gradients), default geometry: 101 tokens,",
         "200 decoder steps (T_out 1000), every length 101 (scripts/tacotron_cbhg_grad_bench.py; medians of %d passes, the autograd passes of %d)" % (args.passes, args.torch_passes),
         "library %s on %s, torch %s" % (L.twv_version().decode(), torch.cuda.get_device_name(0), torch.__version__), ""]
for N in [int(b) for b in args.batches.split(",")]:
    rng = np.random.RandomState(1)
    tok = rng.randint(2, 80, (N, T)).astype(np.int32); tok[:, -1] = 1
    ln = np.full(N, T, np.int32); spk = (np.arange(N) % 2).astype(np.int32)
    TO = STEPS * hp.reduction_factor
    tg = torch.from_numpy(rng.uniform(-4, 4, (N, TO, hp.num_mels)).astype(np.float32)).cuda()
    lt = torch.from_numpy(rng.uniform(-4, 4, (N, TO, hp.num_freq)).astype(np.float32)).cuda()
    m.forward_targets(tok, ln, spk, tg, teacher_forced=True)
    d_mem = torch.from_numpy((rng.randn(N, T, 256) / (N * T)).astype(np.float32)).cuda()
    d_lin = m.linear_loss_cotangent(lt)
    chain_ms = med(lambda: m.loss_gradients(lt), args.passes)
    lines += ["B = %d: the whole chain loss_gradients (linear cotangent, post net, mel cotangent, decoder, encoder) from the host: %.3f ms" % (N, chain_ms)]
    lnd = torch.from_numpy(ln.astype(np.int64)).cuda()
    for side, which, run, Tn in (("encoder", 0, lambda: m.encoder_grad(d_mem), T), ("post net", 1, lambda: m.postnet_grad(d_lin), TO)):
        got = run()
        g = m._grad_cache["encoder" if which == 0 else "post"][1]
        _lib.check(L.twv_tacotron_cbhg_grad_set_timing(g, 1))
        phases = []

        def one():
            run()
            ms = (C.c_double * 4)()
            _lib.check(L.twv_tacotron_cbhg_grad_phase_ms(g, ms))
            phases.append(list(ms))
        call_ms = med(one, args.passes)
        ph = np.median(np.asarray(phases[-args.passes:]), axis=0)
        _lib.check(L.twv_tacotron_cbhg_grad_set_timing(g, 0))
        names = [n for n in got if n not in ("memory", "linear", "d_mel", "d_before_highway", "d_encoder_rnn_init")]
        state = {}
        if which == 0:
            bh = m.workspace_view(N, T, "before_highway").clone().view(N, -1); ei = m.workspace_view(N, T, "encoder_rnn_init").clone().view(N, -1)
            tokd = torch.from_numpy(tok.astype(np.int64)).cuda()

            def auto():
                w = {n: torch.from_numpy(np.asarray(tensors[n], np.float32)).cuda().requires_grad_() for n in names}
                table = torch.cat([torch.zeros_like(w["embedding"][:1]), w["embedding"][1:]], 0)
                x = torch.relu(table[tokd] @ w["prenet/dense_1/kernel"] + w["prenet/dense_1/bias"])
                x = torch.relu(x @ w["prenet/dense_2/kernel"] + w["prenet/dense_2/bias"])
                out = torch_cbhg(w, x, lnd, "encoder_cbhg", hp.enc_bank_size, hp.enc_highway_depth, bh, ei)
                out.backward(d_mem)
                state["g"] = {n: w[n].grad for n in names if not n.endswith("batch_normalization")}
        else:
            mel = m.mel_outputs.clone()
            full = torch.full((N,), TO, dtype=torch.int64, device="cuda")

            def auto():
                w = {n: torch.from_numpy(np.asarray(tensors[n], np.float32)).cuda().requires_grad_() for n in names}
                out = torch_cbhg(w, mel, full, "post_cbhg", hp.post_bank_size, hp.post_highway_depth)
                lin = out @ w[names[-2]] + w[names[-1]]
                lin.backward(d_lin)
                state["g"] = {n: w[n].grad for n in names if not n.endswith("batch_normalization")}
        auto_ms = med(auto, args.torch_passes, warm=1)
        worst = max((float((got[k] - state["g"][k]).abs().max()) / max(float(state["g"][k].abs().max()), 1e-30), k) for k in state["g"])
        total = float(ph.sum())
        lines += ["  %s, %d rows an utterance  (%s)" % (side, Tn, m.cbhg_grad_route("encoder" if which == 0 else "post")),
                  "    recording forward                    %9.3f ms" % ph[0],
                  "    GRUs' backward through time          %9.3f ms   = %.4f ms a step (both directions run side by side)" % (ph[1], ph[1] / Tn),
                  "    row-wise backward (pointwise + dx)   %9.3f ms" % ph[2],
                  "    weight-gradient products             %9.3f ms" % ph[3],
                  "    sum of the phases                    %9.3f ms   (the call from the host, with its allocations: %.3f ms)" % (total, call_ms),
                  "    PyTorch-ROCm float32 autograd, forward + backward of the same graph: %.3f ms  ->  %.2f x the hand-written pass" % (auto_ms, auto_ms / total),
                  "    largest distance between the two gradients, relative to the tensor's maximum: %.2e (%s)" % worst]
    lines.append("")
text = "\n".join(lines)
with open(args.out, "w") as fh:
    fh.write(text)
print(text)
