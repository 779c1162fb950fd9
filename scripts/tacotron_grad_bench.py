#!/usr/bin/env python
"""Times of the Tacotron decoder gradient pass (Tacotron.decoder_grad) at the default geometry: B = 8 and B = 32, 101 tokens, 200 decoder
steps (t_out = 1000), the weights of scripts/tacotron_bench.py.  Per batch: the three phases of twv_tacotron_decoder_grad_run from its own
events (recording forward, backward through time, weight-gradient products), the whole call from the host, and -- the yardstick -- the
PyTorch-ROCm float32 autograd pass (forward + backward) of the same decoder graph on the same device, fed the same memory and initial
states.  Medians of --passes runs.  Writes --out (default profiles/tacotron_decoder_grad_bench.txt).  Needs the GPU."""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np, torch
import twvk_amd
from twvk_amd import _lib
from twvk_amd.tacotron import Tacotron
from tacotron_targets_bench import random_tensors

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tacotron_decoder_grad_bench.txt"))
ap.add_argument("--passes", type=int, default=7)
ap.add_argument("--torch-passes", type=int, default=3)
ap.add_argument("--batches", default="8,32")
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
T, STEPS = 101, 200
GP = "decoder/output_projection_wrapper/multi_rnn_cell/"
AP = "decoder/bahdanau_monotonic_attention/"


def torch_decoder_vjp(w, hp, memory, init, lengths, fed, d_mel):
    """float32 autograd on the device: the teacher-forced decoder (bah_mon_norm) and its backward; returns the leaves' gradients"""
    def gru(x, h, p):
        n = h.shape[1]
        g = torch.sigmoid(torch.cat([x, h], 1) @ w[p + "/gates/kernel"] + w[p + "/gates/bias"])
        r, u = g[:, :n], g[:, n:]
        c = torch.tanh(torch.cat([x, r * h], 1) @ w[p + "/candidate/kernel"] + w[p + "/candidate/bias"])
        return u * h + (1.0 - u) * c
    N, Tn, _ = memory.shape
    AS, DR, L = hp.attention_state_size, hp.dec_rnn_size, hp.dec_layer_num
    mask = torch.arange(Tn, device=memory.device)[None, :] < lengths[:, None]
    values = memory * mask[:, :, None].float()
    keys = values @ w["memory_layer/kernel"]
    v, g_ = w[AP + "attention_v"], w[AP + "attention_g"]
    vh = g_ * v / torch.sqrt((v * v).sum())
    att_h, dec_h = init[:, :AS], [init[:, AS + i * DR:AS + (i + 1) * DR] for i in range(L)]
    context = torch.zeros(N, memory.shape[2], device=memory.device)
    align = torch.zeros(N, Tn, device=memory.device); align[:, 0] = 1.0
    tiny = float(np.finfo(np.float32).tiny)
    # the prenet has no feedback: all steps at once
    frames = torch.cat([torch.zeros_like(fed[:, :1]), fed[:, :-1]], 1)
    p = torch.relu(frames @ w["decoder/decoder_prenet/dense_1/kernel"] + w["decoder/decoder_prenet/dense_1/bias"])
    p = torch.relu(p @ w["decoder/decoder_prenet/dense_2/kernel"] + w["decoder/decoder_prenet/dense_2/bias"])
    ys = []
    for t in range(fed.shape[1]):
        att_h = gru(torch.cat([p[:, t], context], 1), att_h, "decoder/attention_wrapper/gru_cell")
        q = att_h @ w[AP + "query_layer/kernel"]
        score = (vh * torch.tanh(keys + q[:, None, :] + w[AP + "attention_b"])).sum(2) + w[AP + "attention_score_bias"]
        pc = torch.sigmoid(torch.where(mask, score, torch.full_like(score, -float("inf"))))
        lg = torch.log(torch.clamp(1.0 - pc, tiny, 1.0))
        cp = torch.exp(torch.cumsum(lg, 1) - lg)
        align = pc * cp * torch.cumsum(align / torch.clamp(cp, 1e-10, 1.0), 1)
        context = (align[:, None, :] @ values)[:, 0]
        y = torch.cat([att_h, context], 1) @ w[GP + "cell_0/output_projection_wrapper/kernel"] + w[GP + "cell_0/output_projection_wrapper/bias"]
        for i in range(L):
            dec_h[i] = gru(y, dec_h[i], GP + "cell_%d/gru_cell" % (i + 1))
            y = y + dec_h[i]
        ys.append(y)
    out = torch.stack(ys, 1) @ w["decoder/output_projection_wrapper/kernel"] + w["decoder/output_projection_wrapper/bias"]
    mel = out.reshape(N, -1, hp.num_mels)
    mel.backward(d_mel)
    return mel.detach()


def med(fn, passes, warm=2):
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
lines = ["Tacotron decoder gradient pass (Tacotron.decoder_grad), default geometry: 101 tokens, 200 decoder steps (t_out 1000), every length 101",
         "(scripts/tacotron_grad_bench.py; medians of %d passes, the autograd pass of %d)" % (args.passes, args.torch_passes),
         "library %s on %s, torch %s" % (L.twv_version().decode(), torch.cuda.get_device_name(0), torch.__version__), ""]
for N in [int(b) for b in args.batches.split(",")]:
    rng = np.random.RandomState(1)
    tok = rng.randint(2, 80, (N, T)).astype(np.int32); tok[:, -1] = 1
    ln = np.full(N, T, np.int32); spk = (np.arange(N) % 2).astype(np.int32)
    tg = torch.from_numpy(rng.uniform(-4, 4, (N, STEPS * hp.reduction_factor, hp.num_mels)).astype(np.float32)).cuda()
    forced_ms = med(lambda: m.forward_targets(tok, ln, spk, tg, teacher_forced=True), args.passes)
    cot = m.mel_loss_cotangent()
    got = m.decoder_grad(cot)
    _lib.check(L.twv_tacotron_decoder_grad_set_timing(m._grad_cache["decoder"][1], 1))
    phases = []

    def one():
        m.decoder_grad(cot)
        ms = (C.c_double * 3)()
        _lib.check(L.twv_tacotron_decoder_grad_phase_ms(m._grad_cache["decoder"][1], ms))
        phases.append(list(ms))
    call_ms = med(one, args.passes)
    ph = np.median(np.asarray(phases[-args.passes:]), axis=0)
    # the yardstick on the same inputs
    names = [n for n in got if n not in ("d_memory", "d_init", "mel")]
    memory = m.workspace_view(N, T, "memory").clone().view(N, T, -1)
    init = m.workspace_view(N, T, "decoder_init").clone().view(N, -1)
    fed = tg[:, hp.reduction_factor - 1::hp.reduction_factor].contiguous()
    lnd = torch.from_numpy(ln.astype(np.int64)).cuda()
    state = {}

    def auto():
        w = {n: torch.from_numpy(np.asarray(tensors[n], np.float32)).cuda().requires_grad_() for n in names}
        mem, ini = memory.clone().requires_grad_(), init.clone().requires_grad_()
        state["mel"] = torch_decoder_vjp(w, hp, mem, ini, lnd, fed, cot)
        state["g"] = dict({n: w[n].grad for n in names}, d_memory=mem.grad, d_init=ini.grad)
    auto_ms = med(auto, args.torch_passes, warm=1)
    worst = max((float((got[k] - state["g"][k]).abs().max()) / max(float(state["g"][k].abs().max()), 1e-30), k) for k in state["g"])
    total = float(ph.sum())
    lines += ["B = %d  (%s)" % (N, m.decoder_grad_route()),
              "  recording forward          %9.3f ms" % ph[0],
              "  backward through time      %9.3f ms" % ph[1],
              "  weight-gradient products   %9.3f ms" % ph[2],
              "  sum of the phases          %9.3f ms   (the call from the host, with its allocations: %.3f ms)" % (total, call_ms),
              "  for scale: the teacher-forced forward_targets pass of the same batch (encoder, decoder, post net): %.3f ms" % forced_ms,
              "  PyTorch-ROCm float32 autograd, forward + backward of the same decoder graph: %.3f ms  ->  %.2f x the hand-written pass" % (auto_ms, auto_ms / total),
              "  largest distance between the two gradients, relative to the tensor's maximum: %.2e (%s)" % worst, ""]
text = "\n".join(lines)
with open(args.out, "w") as fh:
    fh.write(text)
print(text)
