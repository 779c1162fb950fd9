#!/usr/bin/env python
"""Times of one Tacotron training step (TacotronTrainer.step) at the default geometry: B = 8 and B = 32, 101 tokens, 200
decoder steps (T_out = 1000 frames), the weights of scripts/tacotron_bench.py.  Per batch: the step by phase from events on its stream
(forward_targets + add_loss; the three gradient passes with their range copies; the speaker side; gradient conversion + clip + Adam +
refold + re-pack), the whole step from the host, and -- the yardstick -- the PyTorch-ROCm float32 step of the same evaluation graph on the
same device: forward, autograd backward, clip_grad_norm_(1.0) and torch.optim.Adam over the same trainable tensors.  Medians of --passes
steps.  `--root DIR` (a checkout of the parent commit WITH its built library) adds `infer` of the two builds, processes alternating
(scripts/tacotron_targets_bench.py's measurement).  Writes --out (default profiles/tacotron_train_step_bench.txt).  Needs the GPU.
`--attention_type a,b,...` runs the step at each of these hparams.attention_type values (TacotronTrainer(attention_gradients="any") for
all but the monotonic ones; the PyTorch yardstick restates bah_mon_norm only and runs there alone).  `--json` prints, instead, one line
{"label", "<type> b<N> step_ms" ...}: the per-process record of an A/B of two builds."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np, torch
import torch.nn.functional as F
import twvk_amd
from twvk_amd import _lib
from twvk_amd.tacotron import Tacotron
from twvk_amd.tacotron_train import TacotronTrainer
from tacotron_targets_bench import random_tensors

T, STEPS = 101, 200
GP = "decoder/output_projection_wrapper/multi_rnn_cell/"
AP = "decoder/bahdanau_monotonic_attention/"


def _gru(w, x, h, p):
    n = h.shape[1]
    g = torch.sigmoid(torch.cat([x, h], 1) @ w[p + "/gates/kernel"] + w[p + "/gates/bias"])
    r, u = g[:, :n], g[:, n:]
    c = torch.tanh(torch.cat([x, r * h], 1) @ w[p + "/candidate/kernel"] + w[p + "/candidate/bias"])
    return u * h + (1.0 - u) * c


def torch_cbhg(w, x, lengths, scope, bank, depth, bh=None, init=None):
    """modules.py:25-74 in inference mode (the graph of scripts/tacotron_cbhg_grad_bench.py)"""
    def conv(x, p, relu):
        k = w[p + "/conv1d/kernel"]
        kw = k.shape[0]
        y = F.conv1d(F.pad(x.transpose(1, 2), ((kw - 1) // 2, (kw - 1) - (kw - 1) // 2)), k.permute(2, 1, 0)).transpose(1, 2) + w[p + "/conv1d/bias"]
        y = torch.relu(y) if relu else y
        g, b, m, v = w[p + "/batch_normalization"]
        return (y - m) / torch.sqrt(v + 1e-3) * g + b
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
            hn = _gru(w, y[:, t], h, "%s/bidirectional_rnn/%s/gru_cell" % (scope, d))
            h = torch.where(live, hn, h); o[t] = torch.where(live, hn, torch.zeros_like(hn))
        outs.append(torch.stack(o, 1))
    return torch.cat(outs, 2)


def torch_decoder(w, hp, memory, init, lengths, fed):
    """the teacher-forced decoder, bah_mon_norm (the graph of scripts/tacotron_grad_bench.py)"""
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
    frames = torch.cat([torch.zeros_like(fed[:, :1]), fed[:, :-1]], 1)
    p = torch.relu(frames @ w["decoder/decoder_prenet/dense_1/kernel"] + w["decoder/decoder_prenet/dense_1/bias"])
    p = torch.relu(p @ w["decoder/decoder_prenet/dense_2/kernel"] + w["decoder/decoder_prenet/dense_2/bias"])
    ys = []
    for t in range(fed.shape[1]):
        att_h = _gru(w, torch.cat([p[:, t], context], 1), att_h, "decoder/attention_wrapper/gru_cell")
        q = att_h @ w[AP + "query_layer/kernel"]
        score = (vh * torch.tanh(keys + q[:, None, :] + w[AP + "attention_b"])).sum(2) + w[AP + "attention_score_bias"]
        pc = torch.sigmoid(torch.where(mask, score, torch.full_like(score, -float("inf"))))
        lg = torch.log(torch.clamp(1.0 - pc, tiny, 1.0))
        cp = torch.exp(torch.cumsum(lg, 1) - lg)
        align = pc * cp * torch.cumsum(align / torch.clamp(cp, 1e-10, 1.0), 1)
        context = (align[:, None, :] @ values)[:, 0]
        y = torch.cat([att_h, context], 1) @ w[GP + "cell_0/output_projection_wrapper/kernel"] + w[GP + "cell_0/output_projection_wrapper/bias"]
        for i in range(L):
            dec_h[i] = _gru(w, y, dec_h[i], GP + "cell_%d/gru_cell" % (i + 1))
            y = y + dec_h[i]
        ys.append(y)
    out = torch.stack(ys, 1) @ w["decoder/output_projection_wrapper/kernel"] + w["decoder/output_projection_wrapper/bias"]
    return out.reshape(N, -1, hp.num_mels)


def torch_loss(w, hp, names, tok, lengths, spk, tg, lt):
    """the evaluation graph from the tokens to add_loss's loss (prioritize_loss off), deepvoice with a speaker embedding"""
    soft = lambda t: t / (t.abs() + 1.0)
    e = w["speaker_embedding"][spk]
    sv = [soft(e @ w[("dense" if i == 0 else "dense_%d" % i) + "/kernel"] + w[("dense" if i == 0 else "dense_%d" % i) + "/bias"])
          for i in range(3 + hp.dec_layer_num)]
    table = torch.cat([torch.zeros_like(w["embedding"][:1]), w["embedding"][1:]], 0)
    x = torch.relu(table[tok] @ w["prenet/dense_1/kernel"] + w["prenet/dense_1/bias"])
    x = torch.relu(x @ w["prenet/dense_2/kernel"] + w["prenet/dense_2/bias"])
    memory = torch_cbhg(w, x, lengths, "encoder_cbhg", hp.enc_bank_size, hp.enc_highway_depth, sv[0], sv[1])
    mel = torch_decoder(w, hp, memory, torch.cat(sv[2:], 1), lengths, tg[:, hp.reduction_factor - 1::hp.reduction_factor, :])
    full = torch.full((tg.shape[0],), tg.shape[1], dtype=torch.int64, device=tg.device)
    post = torch_cbhg(w, mel, full, "post_cbhg", hp.post_bank_size, hp.post_highway_depth)
    lin = post @ w[names[-2]] + w[names[-1]]
    return (mel - tg).abs().mean() + (lin - lt).abs().mean()


class TimedTrainer(TacotronTrainer):
    """events at the phase boundaries of a step"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]

    def _forward_done(self): self.ev[1].record()
    def _passes_done(self): self.ev[2].record()
    def _speaker_done(self): self.ev[3].record()

    def step(self, *a, **k):
        self.ev[0].record()
        out = super().step(*a, **k)
        self.ev[4].record()
        return out

    def phases(self):
        self.ev[4].synchronize()
        return [self.ev[i].elapsed_time(self.ev[i + 1]) for i in range(4)]


def infer_ab(parent, rounds, lines):
    """`infer` of the parent build and of this tree, fresh processes alternating"""
    rows = []
    script = os.path.join(ROOT, "scripts", "tacotron_targets_bench.py")
    for i in range(1, rounds + 1):
        for label, root in (("A%d" % i, parent), ("B%d" % i, ROOT)):
            out = subprocess.run([sys.executable, script, "--root", root, "--label", label], capture_output=True, text=True, timeout=300, check=True).stdout
            rows.append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1]))
    lines += ["`infer` of the parent build (A) and of this tree (B), processes alternating A1 B1 A2 B2 ..., each the median of %d passes (ms):" % rows[0]["passes"]]
    for k in ("infer_b8_ms", "infer_b32_ms"):
        a = [r[k] for r in rows if r["label"].startswith("A")]; b = [r[k] for r in rows if r["label"].startswith("B")]
        d = np.median(b) - np.median(a)
        lines += ["  %-12s A: %s  median %.4f   B: %s  median %.4f   B - A %+.4f ms (%+.2f %%), the parent's own spread %.4f ms -> %s"
                  % (k, " ".join("%.4f" % v for v in a), np.median(a), " ".join("%.4f" % v for v in b), np.median(b), d, 100 * d / np.median(a),
                     max(a) - min(a), "inside" if d <= max(a) - min(a) else "OUTSIDE")]
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tacotron_train_step_bench.txt"))
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--torch-passes", type=int, default=2)
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--root", default=None, help="a checkout of the parent commit with its built library: adds the infer A/B")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--attention_type", default="bah_mon_norm")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    hp = twvk_amd.default_hparams()
    L = _lib.lib()
    record = {"label": args.label, "library": L.twv_version().decode()}
    lines = ["One Tacotron training step on the evaluation graph (TacotronTrainer.step: frozen moving statistics, no dropout), default geometry:",
             "101 tokens, 200 decoder steps (T_out 1000), every length 101, two speakers, speaker_embedding_size %d" % hp.speaker_embedding_size,
             "(scripts/tacotron_train_bench.py; medians of %d steps, the PyTorch step of %d)" % (args.passes, args.torch_passes),
             "library %s on %s, torch %s" % (L.twv_version().decode(), torch.cuda.get_device_name(0), torch.__version__), ""]
    for at, N in [(at, int(b)) for at in args.attention_type.split(",") for b in args.batches.split(",")]:
        hp.attention_type = at
        m = Tacotron(hp, num_speakers=2)
        tensors = random_tensors(m.specs)
        m.load_weights(tensors)
        tr = TimedTrainer(m) if at in ("bah_mon_norm", "bah_mon") else TimedTrainer(m, attention_gradients="any")
        rng = np.random.RandomState(1)
        tok = rng.randint(2, 80, (N, T)).astype(np.int32); tok[:, -1] = 1
        ln = np.full(N, T, np.int32); spk = (np.arange(N) % 2).astype(np.int32)
        TO = STEPS * hp.reduction_factor
        tg = torch.from_numpy(rng.uniform(-4, 4, (N, TO, hp.num_mels)).astype(np.float32)).cuda()
        lt = torch.from_numpy(rng.uniform(-4, 4, (N, TO, hp.num_freq)).astype(np.float32)).cuda()
        walls, phases, losses = [], [], []
        for i in range(args.passes + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            losses.append(tr.step(tok, ln, spk, tg, lt)["loss"])
            torch.cuda.synchronize(); walls.append((time.perf_counter() - t0) * 1e3)
            phases.append(tr.phases())
        ph = np.median(np.asarray(phases[1:]), axis=0)
        wall = float(np.median(walls[1:]))
        record["%s b%d step_ms" % (at, N)] = float(ph.sum())
        record["%s b%d gradient_passes_ms" % (at, N)] = float(ph[1])
        if args.json:
            del tr, m
            continue
        # the speaker side alone, its four launches between two events
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        z = [torch.zeros(N, n, device="cuda") for n in (hp.enc_prenet_sizes[1], 2 * hp.enc_rnn_size, hp.attention_state_size + hp.dec_layer_num * hp.dec_rnn_size)]
        spk_us = []
        for i in range(12):
            e0.record(); m._speaker_grad_blob(z[0], z[1], z[2], grad=tr._gblob); e1.record(); torch.cuda.synchronize(); spk_us.append(e0.elapsed_time(e1) * 1e3)
        yard = at == "bah_mon_norm" and args.torch_passes > 0
        auto, first = None, {}
        if yard:
            # the yardstick: the same graph, float32 autograd, clip and Adam of PyTorch
            names = [n for n, _ in m.specs]
            w = {n: torch.from_numpy(np.asarray(tensors[n], np.float32)).cuda() for n in names}
            train = []
            for n in names:
                if n.endswith("batch_normalization"):       # gamma and beta trainable, the moving statistics not
                    gb = w[n][:2].clone().requires_grad_(); train.append(gb); w[n] = torch.cat([gb, w[n][2:]], 0)
                else:
                    w[n].requires_grad_(); train.append(w[n])
            opt = torch.optim.Adam(train, lr=tr.learning_rate(1), betas=(hp.adam_beta1, hp.adam_beta2), eps=1e-8)
            tokd, lnd, spkd = (torch.from_numpy(a.astype(np.int64)).cuda() for a in (tok, ln, spk))

            def torch_step():
                ww = dict(w)
                for n in names:
                    if n.endswith("batch_normalization"):
                        ww[n] = torch.cat([train[names.index(n)], w[n][2:].detach()], 0)
                opt.zero_grad(set_to_none=True)
                loss = torch_loss(ww, hp, names, tokd, lnd, spkd, tg, lt)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(train, 1.0)
                opt.step()
                first.setdefault("loss", float(loss))
            ts = []
            for i in range(args.torch_passes + 1):
                torch.cuda.synchronize(); t0 = time.perf_counter(); torch_step(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
            auto = float(np.median(ts[1:]))
        lines += ["attention_type %s, B = %d   (decoder gradient: %s)" % (at, N, m.decoder_grad_route()),
                  "    forward_targets(teacher_forced) + add_loss            %9.3f ms" % ph[0],
                  "    three gradient passes (post net, decoder, encoder)    %9.3f ms" % ph[1],
                  "    speaker side (twv_tacotron_speaker_grad)              %9.3f ms   (alone, four launches between two events: median %.1f us, min %.1f us)"
                  % (ph[2], float(np.median(spk_us[2:])), float(np.min(spk_us[2:]))),
                  "    gradient conversion + clip + Adam + refold + re-pack  %9.3f ms" % ph[3],
                  "    sum of the phases                                     %9.3f ms   (the step from the host, with its allocations: %.3f ms)" % (float(ph.sum()), wall),
                  "    loss over the timed steps: %s" % " ".join("%.5f" % v for v in losses),
                  ] + (["    PyTorch-ROCm float32: forward + autograd + clip_grad_norm_ + optim.Adam of the same graph: %.3f ms  ->  %.2f x the step (first loss %.5f)"
                        % (auto, auto / wall, first["loss"])] if yard else []) + [""]
        del tr, m
    if args.json:
        print(json.dumps(record))
        return
    if args.root:
        infer_ab(os.path.abspath(args.root), args.ab_rounds, lines)
    text = "\n".join(lines)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
