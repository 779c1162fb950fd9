"""float64 restatement of the reference's Tacotron inference graph for EVERY attention type the port builds (tacotron/tacotron.py:127-144):
the checker of the attention types oracle/ does not cover.  Test infrastructure only.

The graph around the attention mechanism is tests/torch_tacotron_ref.py's (its helpers are imported, not copied); `infer` below is that
module's `infer` with the mechanism made a parameter.  In 'bah_mon_norm' mode it performs the same torch operations in the same order, so
it returns the same bits as torch_tacotron_ref.infer (tests/test_attention_types_cpu.py) -- which is itself cross-checked against
oracle/tacotron.c.  The mechanisms, restated from the reference source and from TensorFlow 1.x's published semantics:
  bah_mon / bah_mon_norm  tf.contrib.seq2seq.BahdanauMonotonicAttention(normalize=False / True): sigmoid(score + score_bias) through
                          monotonic_attention(mode='parallel'); initial alignments one_hot(0)
  bah / bah_norm          tf.contrib.seq2seq.BahdanauAttention(normalize=False / True): softmax over the -inf-masked score; initial
                          alignments zeros (never read)
  luong / luong_scaled    tf.contrib.seq2seq.LuongAttention(scale=False / True): score = (g *) query . keys, no query layer; softmax
  loc_sen                 rnn_wrappers.py:581-727 LocationSensitiveAttention(smoothing=False, cumulate_weights=True): the Bahdanau score
                          v . tanh(keys + W_q q + location_layer(conv31(state)) + b); softmax; state <- alignments + state from zeros;
                          the wrapper attends with, and records, the per-step alignments (rnn_wrappers.py:369-373)
The score is masked with -inf past each length (_maybe_mask_score; memory_sequence_length is given for every type but
bah_mon_norm_hccho, which is not built).  Tolerance checker: float64, whatever order torch picks.
"""
import numpy as np
import torch

import torch_tacotron_ref as R

F64 = R.F64
TYPES = ("bah_mon_norm", "bah_mon", "bah_norm", "bah", "luong", "luong_scaled", "loc_sen")
SCOPE = {"bah_mon_norm": "decoder/bahdanau_monotonic_attention/", "bah_mon": "decoder/bahdanau_monotonic_attention/",
         "bah_norm": "decoder/bahdanau_attention/", "bah": "decoder/bahdanau_attention/", "luong": "decoder/luong_attention/",
         "luong_scaled": "decoder/luong_attention/", "loc_sen": "decoder/Location_Sensitive_Attention/"}


class _Mechanism(object):
    """one attention mechanism: `__call__(query, state) -> (alignments, next_state)` as in TF's AttentionMechanism"""

    def __init__(self, attention_type, w, keys, mask):
        self.type, self.keys, self.mask = attention_type, keys, mask
        ap = SCOPE[attention_type]
        t = attention_type
        if t in ("bah_mon_norm", "bah_mon", "bah_norm", "bah", "loc_sen"):
            self.wq = R._t(w[ap + "query_layer/kernel"])
        if t in ("bah_mon_norm", "bah_norm"):
            v, g = R._t(w[ap + "attention_v"]), R._t(w[ap + "attention_g"])
            self.v = g * v / torch.sqrt((v * v).sum())             # _bahdanau_score(normalize=True): g * v * rsqrt(sum(v^2))
            self.b = R._t(w[ap + "attention_b"])
        elif t in ("bah_mon", "bah"):
            self.v, self.b = R._t(w[ap + "attention_v"]), None
        elif t == "loc_sen":
            self.v, self.b = R._t(w[ap + "attention_variable"]), R._t(w[ap + "attention_bias"])
            self.conv_k = R._t(w[ap + "location_features_convolution/kernel"])           # (31, 1, 32)
            self.conv_b = R._t(w[ap + "location_features_convolution/bias"])
            self.loc_l = R._t(w[ap + "location_features_layer/kernel"])                  # (32, A), no bias
        if t in ("bah_mon_norm", "bah_mon"):
            self.score_bias = R._t(w[ap + "attention_score_bias"])
        self.g = R._t(w[ap + "attention_g"]) if t == "luong_scaled" else None

    def initial_state(self, N, T_in):
        s = torch.zeros(N, T_in, dtype=F64)
        if self.type in ("bah_mon_norm", "bah_mon"):
            s[:, 0] = 1.0                                          # monotonic initial_alignments: one_hot(0)
        return s

    def __call__(self, query, state):
        t = self.type
        if t in ("luong", "luong_scaled"):
            score = (self.keys @ query[:, :, None])[:, :, 0]       # _luong_score: matmul(query, keys, transpose_b=True)
            if self.g is not None:
                score = self.g * score
        else:
            q = query @ self.wq
            arg = self.keys + q[:, None, :]
            if t == "loc_sen":
                f = R._conv1d_same(state[:, :, None], self.conv_k, self.conv_b)          # (N, T, 32), 'same', with bias
                arg = arg + f @ self.loc_l + self.b                # keys + W_query + W_fil + b_a (rnn_wrappers.py:739)
            elif self.b is not None:
                arg = arg + self.b
            score = (self.v * torch.tanh(arg)).sum(dim=2)
            if t in ("bah_mon_norm", "bah_mon"):
                score = score + self.score_bias
        score = torch.where(self.mask, score, torch.full_like(score, -float("inf")))       # _maybe_mask_score(-inf)
        if t in ("bah_mon_norm", "bah_mon"):
            align = R._monotonic_attention_parallel(torch.sigmoid(score), state)          # sigmoid_noise = 0
            return align, align
        align = torch.softmax(score, dim=1)
        return align, (align + state if t == "loc_sen" else align)


@torch.no_grad()
def infer(w, dims, tokens, lengths, speaker_ids, attention_type="bah_mon_norm"):
    """torch_tacotron_ref.infer with the attention mechanism of `attention_type`; returns (mel, linear, alignments) float64 numpy"""
    tokens = np.asarray(tokens); lengths = np.asarray(lengths)
    w = {k: R._t(v) for k, v in w.items()}
    N, T_in = tokens.shape
    multi = dims.n_speakers > 1
    table = R._t(w["embedding"]).clone()
    table[0] = 0.0
    x = table[torch.as_tensor(tokens, dtype=torch.long)]
    before_highway = enc_init = att_init = None
    dec_init = [None] * dims.dec_layers
    embed_to_concat = None
    if multi and getattr(dims, "model_simple", 0) and "speaker_embedding" in w and "dense_1/kernel" not in w:
        embed_to_concat = w["speaker_embedding"][torch.as_tensor(np.asarray(speaker_ids), dtype=torch.long)]
        linear_name = "dense"
    elif multi and "speaker_embedding" not in w:
        ids = torch.as_tensor(np.asarray(speaker_ids), dtype=torch.long)
        before_highway = w["before_highway"][ids]
        enc_init = w["encoder_rnn_init_state"][ids]
        att_init = w["attention_rnn_init_state"][ids]
        dec_init = [w["decoder_rnn_init_states%d" % (i + 1)][ids] for i in range(dims.dec_layers)]
        linear_name = "dense"
    elif multi:
        spk = R._t(w["speaker_embedding"])[torch.as_tensor(np.asarray(speaker_ids), dtype=torch.long)]
        softsign = lambda v: v / (v.abs() + 1.0)
        names = ["dense"] + ["dense_%d" % i for i in range(1, 3 + dims.dec_layers)]
        before_highway = R._dense(spk, w, names[0], softsign)
        enc_init = R._dense(spk, w, names[1], softsign)
        att_init = R._dense(spk, w, names[2], softsign)
        dec_init = [R._dense(spk, w, names[3 + i], softsign) for i in range(dims.dec_layers)]
        linear_name = "dense_%d" % (3 + dims.dec_layers)
    else:
        linear_name = "dense"
    h = R._dense(x, w, "prenet/dense_1", torch.relu)
    h = R._dense(h, w, "prenet/dense_2", torch.relu)
    enc = R._cbhg(h, lengths, w, "encoder_cbhg", dims.enc_bank, 2, dims.enc_hw_depth, before_highway, enc_init)
    mask = torch.as_tensor(np.arange(T_in)[None, :] < lengths[:, None])
    values = enc * mask[:, :, None].to(F64)
    keys = values @ R._t(w["memory_layer/kernel"])
    mech = _Mechanism(attention_type, w, keys, mask)
    RR, M = dims.r, dims.num_mels
    AS = w["decoder/attention_wrapper/gru_cell/candidate/bias"].shape[0]
    att_h = att_init if att_init is not None else torch.zeros(N, AS, dtype=F64)
    dec_h = list(dec_init)
    context = torch.zeros(N, enc.shape[2], dtype=F64)
    state = mech.initial_state(N, T_in)
    frame = torch.zeros(N, M, dtype=F64)
    mel_steps, align_hist = [], []
    gp = "decoder/output_projection_wrapper/multi_rnn_cell/"
    for _step in range(dims.max_iters):
        p = R._dense(frame, w, "decoder/decoder_prenet/dense_1", torch.relu)
        p = R._dense(p, w, "decoder/decoder_prenet/dense_2", torch.relu)
        if embed_to_concat is not None:
            p = torch.cat([p, embed_to_concat], dim=-1)
        att_h = R._gru_cell(torch.cat([p, context], dim=-1), att_h, w, "decoder/attention_wrapper/gru_cell")
        align, state = mech(att_h, state)
        context = (align[:, None, :] @ values)[:, 0]
        align_hist.append(align)
        cat_out = [att_h, context] if embed_to_concat is None else [att_h, context, embed_to_concat]
        y = R._dense(torch.cat(cat_out, dim=-1), w, gp + "cell_0/output_projection_wrapper")
        for i in range(dims.dec_layers):
            if dec_h[i] is None:
                dec_h[i] = torch.zeros(N, y.shape[1], dtype=F64)
            dec_h[i] = R._gru_cell(y, dec_h[i], w, gp + "cell_%d/gru_cell" % (i + 1))
            y = y + dec_h[i]
        out = R._dense(y, w, "decoder/output_projection_wrapper")
        mel_steps.append(out.reshape(N, RR, M))
        frame = out[:, -M:]
    mel = torch.cat(mel_steps, dim=1)
    post = R._cbhg(mel, None, w, "post_cbhg", dims.post_bank, 2, dims.post_hw_depth)
    linear = R._dense(post, w, linear_name)
    alignments = torch.stack(align_hist, dim=2)
    return mel.numpy(), linear.numpy(), alignments.numpy()


class Dims(object):
    """the `dims` infer reads, from hparams"""

    def __init__(self, hp, num_speakers):
        self.n_speakers, self.enc_bank, self.post_bank = num_speakers, hp.enc_bank_size, hp.post_bank_size
        self.enc_hw_depth, self.post_hw_depth, self.dec_layers = hp.enc_highway_depth, hp.post_highway_depth, hp.dec_layer_num
        self.num_mels, self.r, self.max_iters = hp.num_mels, hp.reduction_factor, hp.max_iters
        self.model_simple = 1 if (num_speakers > 1 and getattr(hp, "model_type", "deepvoice") == "simple") else 0


def random_tensors(specs, seed, scale=1.0):
    """seeded weights for a spec list: batch norms near identity, matrices ~ 1/sqrt(fan-in), vectors small; the attention scalars
    and the location filters at sizes that keep the alignments neither flat nor one-hot"""
    rng = np.random.RandomState(seed)
    out = {}
    for name, shp in specs:
        if name.endswith("batch_normalization"):
            c = shp[1]
            out[name] = np.stack([1.0 + 0.1 * rng.randn(c), 0.1 * rng.randn(c), 0.1 * rng.randn(c), 1.0 + 0.2 * rng.rand(c)]).astype(np.float32)
        elif name.endswith("attention_g"):
            out[name] = np.array([0.7 + 0.6 * rng.rand()], np.float32)
        elif name.endswith("attention_score_bias"):
            out[name] = np.array([0.5 * rng.randn()], np.float32)
        elif len(shp) == 1:
            out[name] = (0.1 * rng.randn(*shp)).astype(np.float32)
        else:
            fan = int(np.prod(shp[:-1]))
            s = scale / np.sqrt(fan)
            if name.endswith("location_features_convolution/kernel"):
                s = 2.0 / np.sqrt(fan)
            out[name] = (rng.randn(*shp) * s).astype(np.float32)
    return out
