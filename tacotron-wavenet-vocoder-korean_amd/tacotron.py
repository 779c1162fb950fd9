"""Host-side mirror of the reference's Tacotron inference surface (tacotron/tacotron.py `Tacotron.initialize(...,
rnn_decoder_test_mode=True)` and synthesizer.py `Synthesizer.load / synthesize`) over the HIP C-ABI.

Default hparams path (model_type 'deepvoice' with num_speakers > 1, or a single speaker; attention_type 'bah_mon_norm'), model_type
'simple', and the attention types of ATTENTION_TYPES; tokens in, mel / linear / alignments out.  Text -> token ids (text/*, jamo) and Griffin-Lim are host DSP outside this path."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

BN_EPS = np.float32(1e-3)      # tf.layers.batch_normalization default epsilon
# hparams.attention_type -> twv_tacotron_dims.attention_type (include/twv_amd.h TWV_ATT_*); tacotron.py:127-144.  'gmm' and
# 'bah_mon_norm_hccho' are not built.
ATTENTION_TYPES = {'bah_mon_norm': 0, 'bah_mon': 1, 'bah_norm': 2, 'bah': 3, 'luong': 4, 'luong_scaled': 5, 'loc_sen': 6}
LOC_FILTERS, LOC_KERNEL = 32, 31      # rnn_wrappers.py:662-664 location_features_convolution (filters=32, kernel_size=31)


def _cbhg_specs(scope, cin, bank, bch, proj, pw, depth, rnn):
    s = []
    for k in range(1, bank + 1):
        p = "%s/conv_bank/conv1d_%d/" % (scope, k)
        s += [(p + "conv1d/kernel", (k, cin, bch)), (p + "conv1d/bias", (bch,)), (p + "batch_normalization", (4, bch))]
    c = bank * bch
    for i in range(2):
        p = "%s/proj_%d/" % (scope, i + 1)
        s += [(p + "conv1d/kernel", (pw, c, proj[i])), (p + "conv1d/bias", (proj[i],)), (p + "batch_normalization", (4, proj[i]))]
        c = proj[i]
    if proj[1] != rnn:
        s += [(scope + "/dense/kernel", (proj[1], rnn)), (scope + "/dense/bias", (rnn,))]
    for i in range(depth):
        p = "%s/highway_%d/" % (scope, i + 1)
        s += [(p + "H/kernel", (rnn, rnn)), (p + "H/bias", (rnn,)), (p + "T/kernel", (rnn, rnn)), (p + "T/bias", (rnn,))]
    for dr in ("fw", "bw"):
        p = "%s/bidirectional_rnn/%s/gru_cell/" % (scope, dr)
        s += [(p + "gates/kernel", (2 * rnn, 2 * rnn)), (p + "gates/bias", (2 * rnn,)),
              (p + "candidate/kernel", (2 * rnn, rnn)), (p + "candidate/bias", (rnn,))]
    return s


def _attention_specs(hp):
    """the attention mechanism's tensors (tacotron.py:127-144) after memory_layer/kernel; TF scalars are (1,) here as everywhere"""
    at = getattr(hp, "attention_type", "bah_mon_norm")
    A, AS = hp.attention_size, hp.attention_state_size
    if at == "bah_mon_norm":
        p = "decoder/bahdanau_monotonic_attention/"
        return [(p + "query_layer/kernel", (AS, A)), (p + "attention_v", (A,)), (p + "attention_g", (1,)), (p + "attention_b", (A,)),
                (p + "attention_score_bias", (1,))]
    if at == "bah_mon":            # BahdanauMonotonicAttention(normalize=False): no g, no b; the score bias stays
        p = "decoder/bahdanau_monotonic_attention/"
        return [(p + "query_layer/kernel", (AS, A)), (p + "attention_v", (A,)), (p + "attention_score_bias", (1,))]
    if at == "bah_norm":           # BahdanauAttention(normalize=True)
        p = "decoder/bahdanau_attention/"
        return [(p + "query_layer/kernel", (AS, A)), (p + "attention_v", (A,)), (p + "attention_g", (1,)), (p + "attention_b", (A,))]
    if at == "bah":
        p = "decoder/bahdanau_attention/"
        return [(p + "query_layer/kernel", (AS, A)), (p + "attention_v", (A,))]
    if at in ("luong", "luong_scaled"):
        # LuongAttention has no query layer: the (attention_state_size) cell output is dotted with the (attention_size) keys -- a
        # graph with other sizes fails in TF's matmul
        if AS != A:
            raise ValueError("attention_type %r needs attention_state_size == attention_size (got %d and %d)" % (at, AS, A))
        return [("decoder/luong_attention/attention_g", (1,))] if at == "luong_scaled" else []
    if at == "loc_sen":            # rnn_wrappers.py:647-727 LocationSensitiveAttention
        p = "decoder/Location_Sensitive_Attention/"
        return [(p + "query_layer/kernel", (AS, A)), (p + "location_features_convolution/kernel", (LOC_KERNEL, 1, LOC_FILTERS)),
                (p + "location_features_convolution/bias", (LOC_FILTERS,)), (p + "location_features_layer/kernel", (LOC_FILTERS, A)),
                (p + "attention_variable", (A,)), (p + "attention_bias", (A,))]
    raise NotImplementedError("attention_type %r is not built; built: %s" % (at, ", ".join(ATTENTION_TYPES)))


def tacotron_specs(hp, num_speakers, n_symbols=80):
    """checkpoint tensors (under 'model/inference/') in canonical blob order.  `batch_normalization` entries are (4, C):
    gamma, beta, moving_mean, moving_variance (four TF variables stacked)."""
    E, SE = hp.embedding_size, hp.speaker_embedding_size
    P0, P1 = hp.enc_prenet_sizes
    RN, A, AS, DR, M, R = hp.enc_rnn_size, hp.attention_size, hp.attention_state_size, hp.dec_rnn_size, hp.num_mels, hp.reduction_factor
    ENC = 2 * RN
    s = [("embedding", (n_symbols, E))]
    # tacotron.py:62-104: speaker embedding + the five deep_dense layers exist for num_speakers > 1 only; tf.layers.dense layers
    # are auto-named dense, dense_1, ... in creation order, so the linear-spectrogram layer is "dense" in a single-speaker graph
    dn = ([P1, 2 * RN, AS] + [DR] * hp.dec_layer_num) if num_speakers > 1 else []
    simple = num_speakers > 1 and getattr(hp, "model_type", "deepvoice") == "simple" and SE != 1
    SEc = SE if simple else 0
    if simple:
        # tacotron.py:85-90 model_type 'simple': the speaker embedding only -- it is concatenated to the decoder prenet's output
        # (rnn_wrappers.py:425-432) and to [output, attention] in front of the first projection (:455-463); no dense layers before "dense"
        s += [("speaker_embedding", (num_speakers, SE))]
        dn = []
    elif num_speakers > 1 and SE == 1:
        # tacotron.py:69-75: speaker_embedding_size == 1 -> the five speaker-dependent vectors are embedding tables of their own
        # (modules.py:10-12 get_embed, looked up by speaker id); no speaker embedding, no deep_dense layers (the linear layer is "dense")
        names = ["before_highway", "encoder_rnn_init_state", "attention_rnn_init_state"] + ["decoder_rnn_init_states%d" % (i + 1) for i in range(hp.dec_layer_num)]
        s += [(nm, (num_speakers, n)) for nm, n in zip(names, dn)]
        dn = []
    elif num_speakers > 1:
        s += [("speaker_embedding", (num_speakers, SE))]
    for i, n in enumerate(dn):
        nm = "dense" if i == 0 else "dense_%d" % i
        s += [(nm + "/kernel", (SE, n)), (nm + "/bias", (n,))]
    s += [("prenet/dense_1/kernel", (E, P0)), ("prenet/dense_1/bias", (P0,)), ("prenet/dense_2/kernel", (P0, P1)), ("prenet/dense_2/bias", (P1,))]
    s += _cbhg_specs("encoder_cbhg", P1, hp.enc_bank_size, hp.enc_bank_channel_size, tuple(hp.enc_proj_sizes), hp.enc_proj_width,
                     hp.enc_highway_depth, RN)
    s += [("memory_layer/kernel", (ENC, A))] + _attention_specs(hp)
    D0, D1 = hp.dec_prenet_sizes
    s += [("decoder/decoder_prenet/dense_1/kernel", (M, D0)), ("decoder/decoder_prenet/dense_1/bias", (D0,)),
          ("decoder/decoder_prenet/dense_2/kernel", (D0, D1)), ("decoder/decoder_prenet/dense_2/bias", (D1,))]
    ain = D1 + SEc + ENC
    p = "decoder/attention_wrapper/gru_cell/"
    s += [(p + "gates/kernel", (ain + AS, 2 * AS)), (p + "gates/bias", (2 * AS,)), (p + "candidate/kernel", (ain + AS, AS)), (p + "candidate/bias", (AS,))]
    s += [("decoder/output_projection_wrapper/multi_rnn_cell/cell_0/output_projection_wrapper/kernel", (AS + ENC + SEc, DR)),
          ("decoder/output_projection_wrapper/multi_rnn_cell/cell_0/output_projection_wrapper/bias", (DR,))]
    for i in range(hp.dec_layer_num):
        p = "decoder/output_projection_wrapper/multi_rnn_cell/cell_%d/gru_cell/" % (i + 1)
        s += [(p + "gates/kernel", (2 * DR, 2 * DR)), (p + "gates/bias", (2 * DR,)), (p + "candidate/kernel", (2 * DR, DR)), (p + "candidate/bias", (DR,))]
    s += [("decoder/output_projection_wrapper/kernel", (DR, M * R)), ("decoder/output_projection_wrapper/bias", (M * R,))]
    s += _cbhg_specs("post_cbhg", M, hp.post_bank_size, hp.post_bank_channel_size, tuple(hp.post_proj_sizes), hp.post_proj_width,
                     hp.post_highway_depth, hp.post_rnn_size)
    nm = "dense_%d" % len(dn) if dn else "dense"
    s += [(nm + "/kernel", (2 * hp.post_rnn_size, hp.num_freq)), (nm + "/bias", (hp.num_freq,))]
    return s


def bn_inference_vectors(bn):
    """tf.nn.batch_normalization at inference: inv = rsqrt(var + eps) * gamma ; y = x*inv + (beta - mean*inv)"""
    gamma, beta, mean, var = [np.asarray(v, np.float32) for v in bn]
    inv = (np.float32(1.0) / np.sqrt(var + BN_EPS)).astype(np.float32) * gamma
    shift = (beta - (mean * inv).astype(np.float32)).astype(np.float32)
    return inv.astype(np.float32), shift


def flatten(specs, tensors):
    parts = []
    for n, shp in specs:
        a = np.asarray(tensors[n], np.float32)
        if tuple(a.shape) != tuple(shp):
            raise ValueError("tensor %s has shape %s, expected %s" % (n, a.shape, shp))
        if n.endswith("batch_normalization"):
            parts += list(bn_inference_vectors(a))
        else:
            parts.append(a.reshape(-1))
    return np.concatenate(parts).astype(np.float32)


DECODER_FIRST, DECODER_LAST = "memory_layer/kernel", "decoder/output_projection_wrapper/bias"


def decoder_grad_layout(specs):
    """(name, offset in the canonical blob, shape) of the decoder-side tensors: memory_layer/kernel .. the output projection's bias --
    what Tacotron.decoder_grad returns a gradient for"""
    out, off, on = [], 0, False
    for n, shp in specs:
        size = 2 * shp[1] if n.endswith("batch_normalization") else int(np.prod(shp))     # (flatten: the derived (inv, shift) pair)
        on = on or n == DECODER_FIRST
        if on:
            out.append((n, off, tuple(shp)))
        off += size
        if n == DECODER_LAST:
            break
    return out


def _grad_layout(specs, pick):
    out, off = [], 0
    for i, (n, shp) in enumerate(specs):
        bn = n.endswith("batch_normalization")
        size = 2 * shp[1] if bn else int(np.prod(shp))
        if pick(i, n):
            out.append((n, off, (2, shp[1]) if bn else tuple(shp)))
        off += size
    return out


def encoder_grad_layout(specs):
    """(name, offset in the canonical blob, shape) of the tensors Tacotron.encoder_grad differentiates: embedding, prenet/*, encoder_cbhg/*.
    A batch_normalization entry is the (2, C) slot of the derived (inv, shift) pair (flatten); encoder_grad turns it into (d_gamma, d_beta)."""
    return _grad_layout(specs, lambda i, n: n == "embedding" or n.startswith("prenet/") or n.startswith("encoder_cbhg/"))


def postnet_grad_layout(specs):
    """the same for Tacotron.postnet_grad: post_cbhg/* and the linear-spectrogram layer (the last dense layer of the spec list)"""
    return _grad_layout(specs, lambda i, n: n.startswith("post_cbhg/") or i >= len(specs) - 2)


def speaker_grad_layout(specs):
    """the same for Tacotron.speaker_grad: what lies between embedding and prenet/dense_1/kernel -- the speaker table and its dense layers,
    or the five tables of speaker_embedding_size 1 (nothing for a single speaker)"""
    names = [n for n, _ in specs]
    first, last = names.index("embedding") + 1, names.index("prenet/dense_1/kernel")
    return _grad_layout(specs, lambda i, n: first <= i < last)


def training_layout(specs):
    """(name, offset, shape) of every tensor in the training vector (twv_tacotron_train_floats): the canonical order with a
    batch_normalization entry as its (4, C) checkpoint tensor"""
    out, off = [], 0
    for n, shp in specs:
        out.append((n, off, tuple(shp)))
        off += int(np.prod(shp))
    return out


def flatten_variables(specs, tensors):
    """the training vector of these tensors (flatten without the batch norm folding)"""
    parts = []
    for n, shp in specs:
        a = np.asarray(tensors[n], np.float32)
        if tuple(a.shape) != tuple(shp):
            raise ValueError("tensor %s has shape %s, expected %s" % (n, a.shape, shp))
        parts.append(a.reshape(-1))
    return np.concatenate(parts).astype(np.float32)


def bn_grad_from_inference_pair(pair, raw):
    """a batch norm's gradient as the checkpoint stores the layer: (d_inv, d_shift) of the derived pair (flatten) and the raw (4, C) tensor
    -> (d_gamma, d_beta) as (2, C) float32, float64 inside:
    inv = gamma rsqrt(var + eps), shift = beta - mean inv  =>  d_gamma = rsqrt(var + eps) (d_inv - mean d_shift), d_beta = d_shift"""
    pair, raw = np.asarray(pair, np.float64), np.asarray(raw, np.float64)
    rs = 1.0 / np.sqrt(raw[3] + np.float64(BN_EPS))
    return np.stack([rs * (pair[0] - raw[2] * pair[1]), pair[1]]).astype(np.float32)


# batch norm of the encoder / post-net passes (include/twv_amd.h TWV_BN_*): "inference" = the moving statistics (the evaluation graph),
# "batch" = tf.layers.batch_normalization(training=True), the statistics of the batch over all N * T rows
BN_MODES = {"inference": 0, "batch": 1}
DROPOUT_SITES = {"encoder_prenet_1": 0, "encoder_prenet_2": 1, "decoder_prenet_1": 2, "decoder_prenet_2": 3}
BN_MOMENTUM = 0.99             # tf.layers.batch_normalization's default momentum (modules.py:92-96 passes none)


def dropout_mask_numpy(n, seed, step, site, rate=0.5):
    """twv_dropout_mask restated on the host: n multipliers (float32), element i from (seed, step, site, i) alone"""
    G = np.uint64(0x9E3779B97F4A7C15)

    def mix(z):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))
    with np.errstate(over="ignore"):
        key = mix(np.asarray([seed], np.uint64) + G * np.asarray([4 * int(step) + int(site)], np.uint64))
        z = mix(key + G * np.arange(1, int(n) + 1, dtype=np.uint64))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.where(u >= np.float32(rate), np.float32(1.0 / (1.0 - rate)), np.float32(0.0)).astype(np.float32)


ALIGNMENT_EDITS = {0: "transpose", 1: "argmax one-hot", 2: "squared", 3: "argmax set to 1"}


def alignment_edit_numpy(alignments, mode):
    """twv_tacotron_alignment_edit restated on the host: (B, T_in, steps) alignments as a pass emits them -> the (B, steps, T_in) float32
    feed of infer_manual.  mode 0: the transpose.  With d* = the first step at which encoder row e has its maximum -- every row, the padded
    ones too, so an all-zero row gives step 0 -- mode 1: zeros with a 1 at (d*, e); mode 2: the transpose squared elementwise, not
    renormalised; mode 3: the transpose with a 1 at (d*, e)."""
    if mode not in ALIGNMENT_EDITS:
        raise ValueError("mode must be one of %s, got %r" % (sorted(ALIGNMENT_EDITS), mode))
    a = np.asarray(alignments, np.float32)
    if a.ndim != 3 or 0 in a.shape:
        raise ValueError("alignments must be (B, T_in, steps) with no empty axis, got %s" % (a.shape,))
    t = a.transpose(0, 2, 1).copy()                          # (a copy in any case: with one step the transpose is contiguous as it stands)
    if mode == 0:
        return t
    if mode == 2:
        return t * t
    out = np.zeros_like(t) if mode == 1 else t
    first = a.argmax(axis=2)                                 # (B, T_in): numpy takes the first of equal maxima
    b, e = np.meshgrid(np.arange(a.shape[0]), np.arange(a.shape[1]), indexing="ij")
    out[b, first, e] = np.float32(1.0)
    return out


def moving_average_update(moving, batch, momentum=BN_MOMENTUM):
    """twv_tacotron_moving_update restated on the host, float32: m - (m - batch) * (float32)(1 - momentum)"""
    m, b = np.asarray(moving, np.float32), np.asarray(batch, np.float32)
    return (m - ((m - b).astype(np.float32) * np.float32(1.0 - momentum)).astype(np.float32)).astype(np.float32)


# kind of gradient handle -> (prefix of its C entries, leading arguments of *_create after the model)
_GRAD_KINDS = {"decoder": ("twv_tacotron_decoder_grad", ()), "encoder": ("twv_tacotron_cbhg_grad", (0,)), "post": ("twv_tacotron_cbhg_grad", (1,))}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Tacotron(object):
    """tacotron/tacotron.py `Tacotron(hparams)` + `.initialize(inputs, input_lengths, num_speakers, speaker_id,
    rnn_decoder_test_mode=True)`: after `infer`, `.mel_outputs`, `.linear_outputs`, `.alignments` hold the same tensors."""

    def __init__(self, hparams, num_speakers=2, n_symbols=80, device="cuda:0"):
        hp = self._hparams = hparams
        if hp.attention_type not in ATTENTION_TYPES:
            raise NotImplementedError("attention_type %r is not built; built: %s" % (hp.attention_type, ", ".join(ATTENTION_TYPES)))
        if num_speakers < 1:
            raise NotImplementedError("num_speakers must be >= 1")
        if num_speakers > 1 and hp.model_type not in ('deepvoice', 'simple'):
            raise Exception(" [!] Unkown multi-speaker model type: {}".format(hp.model_type))       # tacotron.py:92
        self.num_speakers = num_speakers
        self.device = torch.device(device)
        self.specs = tacotron_specs(hp, num_speakers, n_symbols)
        d = _lib.TacoDims()
        d.n_symbols, d.embedding_size, d.num_speakers, d.speaker_embedding_size = n_symbols, hp.embedding_size, num_speakers, hp.speaker_embedding_size
        d.enc_prenet_sizes[0], d.enc_prenet_sizes[1] = hp.enc_prenet_sizes
        d.enc_bank_size, d.enc_bank_channel_size = hp.enc_bank_size, hp.enc_bank_channel_size
        d.enc_proj_sizes[0], d.enc_proj_sizes[1] = hp.enc_proj_sizes
        d.enc_proj_width, d.enc_highway_depth, d.enc_rnn_size = hp.enc_proj_width, hp.enc_highway_depth, hp.enc_rnn_size
        d.attention_size, d.attention_state_size = hp.attention_size, hp.attention_state_size
        d.dec_prenet_sizes[0], d.dec_prenet_sizes[1] = hp.dec_prenet_sizes
        d.dec_layer_num, d.dec_rnn_size = hp.dec_layer_num, hp.dec_rnn_size
        d.post_bank_size, d.post_bank_channel_size = hp.post_bank_size, hp.post_bank_channel_size
        d.post_proj_sizes[0], d.post_proj_sizes[1] = hp.post_proj_sizes
        d.post_proj_width, d.post_highway_depth, d.post_rnn_size = hp.post_proj_width, hp.post_highway_depth, hp.post_rnn_size
        d.num_mels, d.reduction_factor, d.num_freq, d.max_iters = hp.num_mels, hp.reduction_factor, hp.num_freq, hp.max_iters
        d.model_simple = 1 if (num_speakers > 1 and hp.model_type == 'simple') else 0
        d.attention_type = ATTENTION_TYPES[hp.attention_type]
        self._dims = d
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.twv_tacotron_create(C.byref(d), C.byref(h)))
        self._h = h
        self._packed = None
        self._ws = None
        self._attention_gradients = "monotonic"

    @property
    def attention_gradients(self):
        """which attention types the decoder gradient (decoder_grad, decoder_grad_forward / _backward, reserve_gradients, loss_gradients,
        variable_gradients, the trainer's step) is made for: "monotonic" -- twv_tacotron_decoder_grad_create: bah_mon_norm and bah_mon,
        every other type refused with TWV_E_UNSUPPORTED -- or "any" -- twv_tacotron_decoder_grad_create_any: every type the model can be
        built with.  "monotonic" is the default only because existing tests pin that refusal.  Setting another value drops the cached
        decoder handle."""
        return self._attention_gradients

    @attention_gradients.setter
    def attention_gradients(self, value):
        if value not in ("monotonic", "any"):
            raise ValueError('attention_gradients must be "monotonic" or "any", got %r' % (value,))
        if value != self._attention_gradients:
            self._drop_grad_handles("decoder")
            self._attention_gradients = value

    def set_option(self, name, value):
        """launch geometry (performance only, results are bit-identical): "decoder_groups" = workgroups per utterance in the decoder
        (0 auto, 1/2/4/8/16, -1 old kernel, 32 XCD-local kernel); "decoder_local" 1/0 = an utterance's workgroups on one XCD (default) or
        spread over the XCDs; "decoder_split_all" -1/0/1 = prenet and query layer split over the workgroups (-1: when local);
        "gemm_group", "gemm_valu", "gemm_timing", "highway_stack" (0: one launch per highway layer) """
        _lib.check(self._L.twv_tacotron_set_option(self._h, name.encode(), int(value)))

    def decoder_kernel_name(self, batch, t_in):
        """the decoder kernel infer() launches for this batch and input length with the options set (a measurement label)"""
        return self._L.twv_tacotron_decoder_kernel_name(self._h, int(batch), int(t_in)).decode()

    def manual_kernel_name(self, batch, t_in):
        """the decoder kernel infer_manual() launches for this batch and input length with the options set ("" where it refuses them)"""
        return self._L.twv_tacotron_manual_kernel_name(self._h, int(batch), int(t_in)).decode()

    def gemm_stats(self):
        """after set_option("gemm_timing", 1): (useful FLOPs, summed kernel milliseconds, launches) of the dense contractions since then"""
        f, ms, n = C.c_double(), C.c_double(), C.c_int64()
        _lib.check(self._L.twv_tacotron_gemm_stats(self._h, C.byref(f), C.byref(ms), C.byref(n)))
        return f.value, ms.value, n.value

    def __del__(self):
        try:
            self._drop_grad_handles()
            if getattr(self, "_h", None):
                self._L.twv_tacotron_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def load_weights(self, tensors):
        blob = flatten(self.specs, tensors)
        # the raw (4, C) batch norm tensors: encoder_grad / postnet_grad turn the derived pair's gradient into (d_gamma, d_beta) with them
        self._bn_raw = {n: np.asarray(tensors[n], np.float64) for n, _ in self.specs if n.endswith("batch_normalization")}
        assert blob.size == self._L.twv_tacotron_blob_floats(self._h), (blob.size, self._L.twv_tacotron_blob_floats(self._h))
        self._train_vec = None                              # (training_vector builds it from the tensors below when a batch-mode pass asks)
        self._train_src = {n: np.asarray(tensors[n], np.float32) for n, _ in self.specs}
        with torch.cuda.device(self.device):
            dblob = self._blob = torch.from_numpy(blob).to(self.device)     # kept: decoder_grad differentiates the canonical tensors
            self._packed = torch.empty(self._L.twv_tacotron_packed_bytes(self._h) // 4, dtype=torch.float32, device=self.device)
            _lib.check(self._L.twv_tacotron_pack(self._h, _ptr(dblob), _ptr(self._packed), _stream()))
            torch.cuda.current_stream().synchronize()

    def infer(self, inputs, input_lengths, speaker_id, want_linear=True, want_alignments=True):
        hp = self._hparams
        with torch.cuda.device(self.device):
            tok = torch.as_tensor(np.asarray(inputs, np.int32), device=self.device).contiguous()
            N, T = tok.shape
            ln = torch.as_tensor(np.asarray(input_lengths, np.int32), device=self.device).contiguous()
            sp = None                                        # synthesizer.py:150-151: no speaker_id feed for a single-speaker model
            if self.num_speakers > 1:
                sp = torch.as_tensor(np.asarray(speaker_id, np.int32), device=self.device).contiguous()
            need = self._L.twv_tacotron_workspace_bytes(self._h, N, T) // 4
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.float32, device=self.device)
            TO = hp.max_iters * hp.reduction_factor
            mel = torch.empty((N, TO, hp.num_mels), dtype=torch.float32, device=self.device)
            lin = torch.empty((N, TO, hp.num_freq), dtype=torch.float32, device=self.device) if want_linear else None
            al = torch.empty((N, T, hp.max_iters), dtype=torch.float32, device=self.device) if want_alignments else None
            status = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self._L.twv_tacotron_infer(self._h, _ptr(self._packed), _ptr(tok), _ptr(ln), _ptr(sp), N, T, _ptr(self._ws),
                                                  _ptr(mel), _ptr(lin), _ptr(al), _ptr(status), _stream()))
        self.inputs, self.input_lengths, self.speaker_id = tok, ln, sp
        self.mel_outputs, self.linear_outputs, self.alignments = mel, lin, al
        self.mel_targets = None                              # (the outputs no longer belong to a pass with targets: add_loss refuses)
        return mel, lin, al

    def infer_manual(self, inputs, input_lengths, speaker_id, manual_alignments, want_linear=True, want_alignments=True):
        """the inference graph fed `is_manual_attention: True, manual_alignments: ...` (tacotron.py:122-123, synthesizer.py:146-147): at
        decoder step t the attention wrapper uses manual_alignments[:, t, :] in place of what its mechanism computes (rnn_wrappers.py:
        369-374), exactly as given -- no mask past the lengths, no normalisation.  manual_alignments: (B, steps, T_in) array or device
        tensor, 1 <= steps <= max_iters; the decoder runs free for `steps` steps.  Returns what infer returns, at `steps`: mel
        (B, steps * r, num_mels), linear (B, steps * r, num_freq), alignments (B, T_in, steps) = the manual values transposed.  Runs on the
        split kernel or (decoder_groups = -1) the single-workgroup kernel, never the XCD-local one: decoder_groups = 32 raises."""
        hp = self._hparams
        with torch.cuda.device(self.device):
            tok = self._device_i32(inputs)
            N, T = tok.shape
            ln = self._device_i32(input_lengths)
            sp = None
            if self.num_speakers > 1:
                sp = self._device_i32(speaker_id)
            if not torch.is_tensor(manual_alignments):
                manual_alignments = torch.from_numpy(np.ascontiguousarray(manual_alignments, np.float32))
            man = manual_alignments.to(device=self.device, dtype=torch.float32).contiguous()
            if man.dim() != 3 or man.shape[0] != N or man.shape[2] != T or man.shape[1] < 1:
                raise ValueError("manual_alignments must be (%d, steps >= 1, %d), got %s" % (N, T, tuple(man.shape)))
            steps = int(man.shape[1])                            # (steps above max_iters are refused by the library)
            need = self._L.twv_tacotron_workspace_bytes(self._h, N, T) // 4
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.float32, device=self.device)
            TO = steps * hp.reduction_factor
            mel = torch.empty((N, TO, hp.num_mels), dtype=torch.float32, device=self.device)
            lin = torch.empty((N, TO, hp.num_freq), dtype=torch.float32, device=self.device) if want_linear else None
            al = torch.empty((N, T, steps), dtype=torch.float32, device=self.device) if want_alignments else None
            status = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self._L.twv_tacotron_infer_manual(self._h, _ptr(self._packed), _ptr(tok), _ptr(ln), _ptr(sp), N, T, _ptr(man), steps,
                                                         _ptr(self._ws), _ptr(mel), _ptr(lin), _ptr(al), _ptr(status), _stream()))
        self.inputs, self.input_lengths, self.speaker_id = tok, ln, sp
        self.mel_outputs, self.linear_outputs, self.alignments = mel, lin, al
        self.mel_targets = None
        return mel, lin, al

    def edit_alignments(self, alignments, mode):
        """synthesizer.py:165-190 on the device (twv_tacotron_alignment_edit; alignment_edit_numpy is the same on the host): the (B, T_in,
        steps) alignments of a pass, array or device tensor -> the (B, steps, T_in) device tensor infer_manual takes.  mode 0 transposes,
        1 = one-hot at every encoder row's argmax over the steps, 2 = squared ("sharpening"), 3 = that argmax set to 1."""
        with torch.cuda.device(self.device):
            if not torch.is_tensor(alignments):
                alignments = torch.from_numpy(np.ascontiguousarray(alignments, np.float32))
            al = alignments.to(device=self.device, dtype=torch.float32).contiguous()
            if al.dim() != 3:
                raise ValueError("alignments must be (B, T_in, steps), got %s" % (tuple(al.shape),))
            N, T, steps = (int(v) for v in al.shape)
            out = torch.empty((N, steps, T), dtype=torch.float32, device=self.device)
            _lib.check(self._L.twv_tacotron_alignment_edit(_ptr(al), N, T, steps, int(mode), _ptr(out), _stream()))
        return out

    def forward_targets(self, inputs, input_lengths, speaker_id, mel_targets, teacher_forced=False, want_linear=True, want_alignments=True):
        """`.initialize(inputs, input_lengths, num_speakers, speaker_id, mel_targets, ...)` (tacotron.py:36-37): the decoder under
        TacoTrainingHelper (helpers.py:44-87) for mel_targets.shape[1] / r steps.  teacher_forced=False is the reference's test_model
        (rnn_decoder_test_mode=True: free-running, the targets give the length only); teacher_forced=True feeds step t >= 1 the target
        frame t*r - 1.  Every layer stays in inference mode in both (no dropout, moving-average batch norm: the reference's training-mode
        layers belong to a training step).  mel_targets: (N, T_out, num_mels) array or tensor, T_out a multiple of r, T_out / r <= max_iters.
        inputs, input_lengths and speaker_id: arrays, or int32 tensors -- a batch already on the device (tacotron_feed.BatchStager) is
        used where it lies, with no host round trip."""
        hp = self._hparams
        with torch.cuda.device(self.device):
            tok = self._device_i32(inputs)
            N, T = tok.shape
            ln = self._device_i32(input_lengths)
            sp = None
            if self.num_speakers > 1:
                sp = self._device_i32(speaker_id)
            if not torch.is_tensor(mel_targets):
                mel_targets = torch.from_numpy(np.ascontiguousarray(mel_targets, np.float32))
            tgt = mel_targets.to(device=self.device, dtype=torch.float32).contiguous()
            if tgt.dim() != 3 or tgt.shape[0] != N or tgt.shape[2] != hp.num_mels:
                raise ValueError("mel_targets must be (%d, T_out, %d), got %s" % (N, hp.num_mels, tuple(tgt.shape)))
            TO = int(tgt.shape[1])
            if TO < 1:
                raise ValueError("mel_targets has no frames: T_out / r decoder steps must satisfy 1 <= steps <= max_iters")
            steps = TO // hp.reduction_factor                    # (a T_out the library refuses is refused there, before this is used)
            need = self._L.twv_tacotron_workspace_bytes(self._h, N, T) // 4
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.float32, device=self.device)
            mel = torch.empty((N, TO, hp.num_mels), dtype=torch.float32, device=self.device)
            lin = torch.empty((N, TO, hp.num_freq), dtype=torch.float32, device=self.device) if want_linear else None
            al = torch.empty((N, T, max(steps, 1)), dtype=torch.float32, device=self.device) if want_alignments else None
            status = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self._L.twv_tacotron_forward_targets(self._h, _ptr(self._packed), _ptr(tok), _ptr(ln), _ptr(sp), N, T, _ptr(tgt), TO,
                                                            1 if teacher_forced else 0, _ptr(self._ws), _ptr(mel), _ptr(lin), _ptr(al),
                                                            _ptr(status), _stream()))
        self.inputs, self.input_lengths, self.speaker_id = tok, ln, sp
        self.mel_outputs, self.linear_outputs, self.alignments, self.mel_targets = mel, lin, al, tgt
        self._teacher_forced = bool(teacher_forced)
        return mel, lin, al

    def _forced_pass(self, what):
        if getattr(self, "mel_targets", None) is None or not getattr(self, "_teacher_forced", False):
            raise ValueError("%s needs a forward_targets pass with teacher_forced=True first" % what)
        return self.mel_outputs, self.mel_targets

    def mel_loss_cotangent(self, loss_coeff=None):
        """d(mel term of add_loss) / d mel_outputs on the last teacher-forced forward_targets pass (tacotron.py:258-282):
        sign(mel - target) * loss_coeff[n] / (N * T_out * num_mels), a (N, T_out, num_mels) tensor on the device."""
        mel, tgt = self._forced_pass("mel_loss_cotangent")
        N, TO, M = (int(v) for v in mel.shape)
        with torch.cuda.device(self.device):
            co = self._loss_coeff(loss_coeff, N)
            out = torch.empty_like(mel)
            _lib.check(self._L.twv_tacotron_mel_loss_grad(_ptr(mel), _ptr(tgt), _ptr(co), N, TO, M, _ptr(out), _stream()))
        return out

    def workspace_view(self, batch, t_in, which):
        """the piece `which` ("memory", "keys", "decoder_init"; "before_highway", "encoder_rnn_init" of a multi-speaker model) of the workspace the last pass of (batch, t_in) used, as a flat view"""
        off, n = C.c_longlong(), C.c_longlong()
        _lib.check(self._L.twv_tacotron_workspace_view(self._h, int(batch), int(t_in), which.encode(), C.byref(off), C.byref(n)))
        return self._ws[off.value:off.value + n.value]

    def decoder_grad(self, d_mel, prenet_masks=None):
        """The vector-Jacobian product of the teacher-forced decoder of the last forward_targets(teacher_forced=True) pass: d_mel
        (N, T_out, num_mels) is the cotangent on the mel output; memory and the initial states are read from that pass's workspace.
        prenet_masks: None (the evaluation graph) or two (N, steps, dec_prenet_sizes[i]) arrays of multipliers applied after the decoder
        prenet's relus (dropout: 0 or 1 / keep_prob).  Returns a dict: every decoder-side checkpoint tensor's gradient by name (TF scalars
        as (1,)), "d_memory" (N, T_in, 2 * enc_rnn_size), "d_init" (N, attention_state_size + dec_layer_num * dec_rnn_size) and "mel", the
        recorded forward's output -- device tensors."""
        grad, d_memory, d_init, mel_out = self._decoder_grad_blob(d_mel, prenet_masks)
        with torch.cuda.device(self.device):
            out = self._named_grads(grad, decoder_grad_layout(self.specs))       # (no batch norm on the decoder side)
        out.update({"d_memory": d_memory, "d_init": d_init, "mel": mel_out})
        return out

    def _decoder_grad_blob(self, d_mel, prenet_masks=None):
        """decoder_grad's pass with the gradient as the C entry leaves it: (blob-shaped gradient, d_memory, d_init, mel)"""
        hp = self._hparams
        mel, tgt = self._forced_pass("decoder_grad")
        if getattr(self, "_blob", None) is None:
            raise ValueError("decoder_grad needs load_weights first")
        N, TO, M = (int(v) for v in tgt.shape)
        T = int(self.inputs.shape[1])
        steps = TO // hp.reduction_factor
        with torch.cuda.device(self.device):
            dm = self._device_f32(d_mel, (N, TO, M), "d_mel must be %s, got %s")
            masks = self._prenet_masks(prenet_masks, (N, steps), hp.dec_prenet_sizes)
            g, ws = self._grad_handle("decoder", (N, T, steps))
            ENC, ninit = 2 * hp.enc_rnn_size, hp.attention_state_size + hp.dec_layer_num * hp.dec_rnn_size
            memory, init = self.workspace_view(N, T, "memory"), self.workspace_view(N, T, "decoder_init")
            mel_out = torch.empty((N, TO, M), dtype=torch.float32, device=self.device)
            grad = torch.empty_like(self._blob)
            d_memory = torch.empty((N, T, ENC), dtype=torch.float32, device=self.device)
            d_init = torch.empty((N, ninit), dtype=torch.float32, device=self.device)
            status = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self._L.twv_tacotron_decoder_grad_run(g, _ptr(self._blob), _ptr(memory), _ptr(init), _ptr(self.input_lengths),
                                                             _ptr(tgt), _ptr(dm), _ptr(masks[0]), _ptr(masks[1]), _ptr(ws),
                                                             _ptr(status), _stream(), _ptr(mel_out), _ptr(grad), _ptr(d_memory), _ptr(d_init)))
        return grad, d_memory, d_init, mel_out

    def decoder_grad_route(self):
        """the label of the gradient kernels of the last decoder_grad call ('' before one)"""
        return self._grad_route("decoder")

    def cbhg_grad_route(self, which):
        """the label of the gradient kernels of the last encoder_grad (which = "encoder") / postnet_grad ("post") call ('' before one)"""
        if which not in ("encoder", "post"):
            raise KeyError(which)
        return self._grad_route(which)

    # ---- what the gradient methods share
    def _grad_handle(self, kind, sizes):
        """(handle, workspace) of a kind of _GRAD_KINDS at `sizes` (the arguments of its *_create).  One handle per kind lives as long as
        the model: when the sizes change it is reshaped (*_reshape keeps its rocBLAS handle, events and device buffers; a refusal leaves
        it and this cache as they were), and its workspace tensor only ever grows."""
        cache = self.__dict__.setdefault("_grad_cache", {})
        entry = cache.get(kind)
        prefix, lead = _GRAD_KINDS[kind]
        if entry is None:
            g, ws = C.c_void_p(), None
            create = "_create_any" if kind == "decoder" and self._attention_gradients == "any" else "_create"
            _lib.check(getattr(self._L, prefix + create)(self._h, *(lead + tuple(sizes) + (C.byref(g),))))
        else:
            g, ws = entry[1:]
            if entry[0] != sizes:
                _lib.check(getattr(self._L, prefix + "_reshape")(g, *sizes))
        cache[kind] = (sizes, g, ws)                     # (the cache says what the handle is at, also when the allocation below fails)
        need = max(getattr(self._L, prefix + "_workspace_bytes")(g) // 4, getattr(self, "_grad_reserve", {}).get(kind, 0))
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.float32, device=self.device)
            cache[kind] = (sizes, g, ws)
        return g, ws

    def reserve_gradients(self, batch, t_in, steps):
        """sizes the three gradient workspaces once for the largest batch a feeder can produce -- (batch, t_in) tokens, steps decoder steps
        = steps * r target frames: no later pass of at most these sizes allocates (a workspace's size grows with each of its sizes).
        The reservation outlives the handles."""
        hp = self._hparams
        reserve = self.__dict__.setdefault("_grad_reserve", {})
        batch, t_in, steps = int(batch), int(t_in), int(steps)
        with torch.cuda.device(self.device):
            for kind, sizes in (("decoder", (batch, t_in, steps)), ("encoder", (batch, t_in)), ("post", (batch, steps * hp.reduction_factor))):
                _, ws = self._grad_handle(kind, sizes)
                reserve[kind] = max(reserve.get(kind, 0), ws.numel())

    def _drop_grad_handles(self, kind=None):
        cache = getattr(self, "_grad_cache", {})
        for k in [k for k in list(cache) if kind in (None, k)]:
            getattr(self._L, _GRAD_KINDS[k][0] + "_destroy")(cache.pop(k)[1])

    def _grad_route(self, kind):
        entry = getattr(self, "_grad_cache", {}).get(kind)
        return getattr(self._L, _GRAD_KINDS[kind][0] + "_route")(entry[1]).decode() if entry else ""

    def _device_i32(self, value):
        """array or tensor -> contiguous int32 tensor on the device (a device tensor of that kind is returned as it is)"""
        if torch.is_tensor(value):
            return value.to(device=self.device, dtype=torch.int32).contiguous()
        return torch.as_tensor(np.asarray(value, np.int32), device=self.device).contiguous()

    def _device_f32(self, value, shape, message):
        """array or tensor -> contiguous float32 tensor on the device; ValueError(message % (shape, its shape)) when a shape is given and is not its shape"""
        if not torch.is_tensor(value):
            value = torch.from_numpy(np.ascontiguousarray(value, np.float32))
        t = value.to(device=self.device, dtype=torch.float32).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(message % (tuple(shape), tuple(t.shape)))
        return t

    def _prenet_masks(self, prenet_masks, lead, sizes):
        """None, or the two dropout multipliers of a prenet as device tensors of lead + (sizes[i],)"""
        if prenet_masks is None:
            return [None, None]
        return [self._device_f32(prenet_masks[i], lead + (sizes[i],), "prenet_masks[%d] must be %%s, got %%s" % i) for i in range(2)]

    def _loss_coeff(self, loss_coeff, N):
        """add_loss's per-utterance factors on the device (ones when None)"""
        if torch.is_tensor(loss_coeff):
            co = loss_coeff.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
            if tuple(co.shape) != (N,):
                raise ValueError("loss_coeff must hold one factor per utterance (%d), got shape %s" % (N, tuple(co.shape)))
            return co
        co = np.ones(N, np.float32) if loss_coeff is None else np.asarray(loss_coeff, np.float32).reshape(-1)
        if co.shape != (N,):
            raise ValueError("loss_coeff must hold one factor per utterance (%d), got shape %s" % (N, co.shape))
        return torch.from_numpy(co).to(self.device)

    def _named_grads(self, grad, layout, mode="inference"):
        """the blob-shaped gradient as a dict by checkpoint name, a batch norm's slot as (d_gamma, d_beta): what a batch-mode pass wrote
        there, or the inference mode's (d_inv, d_shift) through bn_grad_from_inference_pair"""
        out = {}
        for name, off, shp in layout:
            t = grad[off:off + int(np.prod(shp))].view(*shp)
            if name.endswith("batch_normalization") and mode != "batch":
                t = torch.from_numpy(bn_grad_from_inference_pair(t.cpu().numpy(), self._bn_raw[name])).to(self.device)
            out[name] = t
        return out

    # ---- batch-statistics mode and the passes' halves
    def training_vector(self):
        """the training vector (flatten_variables: batch norms as their (4, C) tensors) on the device: what a batch-mode pass reads gamma and
        beta from.  Built from the tensors of load_weights; a TacotronTrainer puts its own vector here, which its steps update."""
        if getattr(self, "_train_vec", None) is None:
            if getattr(self, "_train_src", None) is None:
                raise ValueError("batch mode needs load_weights first")
            with torch.cuda.device(self.device):
                self._train_vec = torch.from_numpy(flatten_variables(self.specs, self._train_src)).to(self.device)
        return self._train_vec

    def _cbhg_handle(self, kind, sizes, mode):
        """_grad_handle of "encoder" / "post" put into `mode`"""
        if mode not in BN_MODES:
            raise ValueError("mode must be one of %s, got %r" % (sorted(BN_MODES), mode))
        g, ws = self._grad_handle(kind, sizes)
        _lib.check(self._L.twv_tacotron_cbhg_grad_set_mode(g, BN_MODES[mode], _ptr(self.training_vector()) if mode == "batch" else None))
        self.__dict__.setdefault("_bn_mode", {})[kind] = mode
        return g, ws

    def batch_statistics(self, which):
        """the statistics of the last batch-mode pass of `which` ("encoder" / "post"): {batch_normalization name: (2, C) device tensor =
        (mean, biased variance) over all N * T rows of that batch norm's input}"""
        if which not in ("encoder", "post"):
            raise KeyError(which)
        return self._split_stats(self._batch_stats_flat(which), which)

    def _batch_stats_flat(self, which):
        entry = getattr(self, "_grad_cache", {}).get(which)
        if entry is None:
            raise ValueError("batch_statistics needs a batch-mode pass first")
        with torch.cuda.device(self.device):
            out = torch.empty(self._L.twv_tacotron_cbhg_grad_batch_stats_floats(entry[1]), dtype=torch.float32, device=self.device)
            _lib.check(self._L.twv_tacotron_cbhg_grad_batch_stats(entry[1], _ptr(out), _stream()))
        return out

    def _split_stats(self, flat, which):
        scope = "encoder_cbhg/" if which == "encoder" else "post_cbhg/"
        out, off = {}, 0
        for n, shp in self.specs:
            if n.startswith(scope) and n.endswith("batch_normalization"):
                out[n] = flat[off:off + 2 * shp[1]].view(2, shp[1])
                off += 2 * shp[1]
        assert off == flat.numel(), (off, flat.numel())
        return out

    def dropout_mask(self, shape, seed, step, site, rate=0.5):
        """dropout multipliers of `shape` on the device (twv_dropout_mask): 1 / (1 - rate) where kept, 0 where dropped; an element depends
        on (seed, step, site, its index) alone.  site: a key of DROPOUT_SITES or 0 .. 3.  dropout_mask_numpy gives the same bits."""
        site = DROPOUT_SITES.get(site, site)
        with torch.cuda.device(self.device):
            out = torch.empty(tuple(int(v) for v in shape), dtype=torch.float32, device=self.device)
            _lib.check(self._L.twv_dropout_mask(_ptr(out), out.numel(), int(seed), int(step), int(site), float(rate), _stream()))
        return out

    def encoder_grad_forward(self, prenet_masks=None, mode="inference"):
        """the recording forward of encoder_grad alone, on the tokens of the last forward_targets(teacher_forced=True) pass: returns memory
        (N, T_in, 2 * enc_rnn_size).  encoder_grad_backward(d_memory) finishes the pass."""
        hp = self._hparams
        self._forced_pass("encoder_grad_forward")
        if getattr(self, "_blob", None) is None:
            raise ValueError("encoder_grad_forward needs load_weights first")
        N, T = (int(v) for v in self.inputs.shape)
        with torch.cuda.device(self.device):
            masks = self._prenet_masks(prenet_masks, (N, T), hp.enc_prenet_sizes)
            g, ws = self._cbhg_handle("encoder", (N, T), mode)      # (first: a model the pass is not built for is refused in the library's words)
            bh = init = None
            if self.num_speakers > 1:
                bh, init = self.workspace_view(N, T, "before_highway"), self.workspace_view(N, T, "encoder_rnn_init")
            memory = torch.empty((N, T, 2 * hp.enc_rnn_size), dtype=torch.float32, device=self.device)
            status = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self._L.twv_tacotron_encoder_grad_forward(g, _ptr(self._blob), _ptr(self.inputs), _ptr(self.input_lengths), _ptr(bh), _ptr(init),
                                                                 _ptr(masks[0]), _ptr(masks[1]), _ptr(ws), _ptr(status), _stream(), _ptr(memory)))
        self._enc_half = (N, T, bh is not None)
        return memory

    def encoder_grad_backward(self, d_memory):
        """the backward of the last encoder_grad_forward: (blob-shaped gradient, d_before_highway, d_encoder_rnn_init); in batch mode a batch
        norm's slot of the gradient holds (d_gamma, d_beta), in inference mode (d_inv, d_shift)"""
        hp = self._hparams
        if getattr(self, "_enc_half", None) is None:
            raise ValueError("encoder_grad_backward needs encoder_grad_forward first")
        N, T, spk = self._enc_half
        ENC = 2 * hp.enc_rnn_size
        with torch.cuda.device(self.device):
            dm = self._device_f32(d_memory, (N, T, ENC), "d_memory must be %s, got %s")
            g, ws = self._grad_handle("encoder", (N, T))
            d_bh = torch.empty((N, hp.enc_prenet_sizes[1]), dtype=torch.float32, device=self.device) if spk else None
            d_init = torch.empty((N, ENC), dtype=torch.float32, device=self.device) if spk else None
            grad = torch.empty_like(self._blob)
            status = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self._L.twv_tacotron_encoder_grad_backward(g, _ptr(self._blob), _ptr(self.inputs), _ptr(self.input_lengths), _ptr(dm), _ptr(ws),
                                                                  _ptr(status), _stream(), _ptr(grad), _ptr(d_bh), _ptr(d_init)))
        return grad, d_bh, d_init

    def postnet_grad_forward(self, mel, mode="inference"):
        """the recording forward of postnet_grad alone: mel (N, T_out, num_mels) -> linear (N, T_out, num_freq)"""
        hp = self._hparams
        if getattr(self, "_blob", None) is None:
            raise ValueError("postnet_grad_forward needs load_weights first")
        with torch.cuda.device(self.device):
            mel = self._device_f32(mel, None, "")
            if mel.dim() != 3 or int(mel.shape[2]) != hp.num_mels:
                raise ValueError("mel must be (N, T_out, %d), got %s" % (hp.num_mels, tuple(mel.shape)))
            N, TO, _ = (int(v) for v in mel.shape)
            g, ws = self._cbhg_handle("post", (N, TO), mode)
            lin = torch.empty((N, TO, hp.num_freq), dtype=torch.float32, device=self.device)
            status = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self._L.twv_tacotron_postnet_grad_forward(g, _ptr(self._blob), _ptr(mel), _ptr(ws), _ptr(status), _stream(), _ptr(lin)))
        self._post_half = mel
        return lin

    def postnet_grad_backward(self, d_linear):
        """the backward of the last postnet_grad_forward: (blob-shaped gradient, d_mel)"""
        hp = self._hparams
        mel = getattr(self, "_post_half", None)
        if mel is None:
            raise ValueError("postnet_grad_backward needs postnet_grad_forward first")
        N, TO, _ = (int(v) for v in mel.shape)
        with torch.cuda.device(self.device):
            dl = self._device_f32(d_linear, (N, TO, hp.num_freq), "d_linear must be %s, got %s")
            g, ws = self._grad_handle("post", (N, TO))
            grad, d_mel = torch.empty_like(self._blob), torch.empty_like(mel)
            status = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self._L.twv_tacotron_postnet_grad_backward(g, _ptr(self._blob), _ptr(mel), _ptr(dl), _ptr(ws), _ptr(status), _stream(),
                                                                  _ptr(grad), _ptr(d_mel)))
        return grad, d_mel

    def decoder_grad_forward(self, memory=None, prenet_masks=None):
        """the recording forward of decoder_grad alone, teacher-forced on the targets of the last forward_targets(teacher_forced=True) pass:
        memory (N, T_in, 2 * enc_rnn_size), by default that pass's; the initial states are that pass's.  Returns mel (N, T_out, num_mels)."""
        hp = self._hparams
        _, tgt = self._forced_pass("decoder_grad_forward")
        if getattr(self, "_blob", None) is None:
            raise ValueError("decoder_grad_forward needs load_weights first")
        N, TO, M = (int(v) for v in tgt.shape)
        T = int(self.inputs.shape[1])
        steps = TO // hp.reduction_factor
        with torch.cuda.device(self.device):
            masks = self._prenet_masks(prenet_masks, (N, steps), hp.dec_prenet_sizes)
            g, ws = self._grad_handle("decoder", (N, T, steps))
            mem = self.workspace_view(N, T, "memory") if memory is None else self._device_f32(memory, (N, T, 2 * hp.enc_rnn_size), "memory must be %s, got %s")
            init = self.workspace_view(N, T, "decoder_init").clone()
            mel_out = torch.empty((N, TO, M), dtype=torch.float32, device=self.device)
            status = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self._L.twv_tacotron_decoder_grad_forward(g, _ptr(self._blob), _ptr(mem), _ptr(init), _ptr(self.input_lengths), _ptr(tgt),
                                                                 _ptr(masks[0]), _ptr(masks[1]), _ptr(ws), _ptr(status), _stream(), _ptr(mel_out)))
        self._dec_half = (N, T, steps, mem, init)
        return mel_out

    def decoder_grad_backward(self, d_mel):
        """the backward of the last decoder_grad_forward: (blob-shaped gradient, d_memory, d_init)"""
        hp = self._hparams
        if getattr(self, "_dec_half", None) is None:
            raise ValueError("decoder_grad_backward needs decoder_grad_forward first")
        N, T, steps, mem, init = self._dec_half
        with torch.cuda.device(self.device):
            dm = self._device_f32(d_mel, (N, steps * hp.reduction_factor, hp.num_mels), "d_mel must be %s, got %s")
            g, ws = self._grad_handle("decoder", (N, T, steps))
            grad = torch.empty_like(self._blob)
            d_memory = torch.empty((N, T, 2 * hp.enc_rnn_size), dtype=torch.float32, device=self.device)
            d_init = torch.empty((N, hp.attention_state_size + hp.dec_layer_num * hp.dec_rnn_size), dtype=torch.float32, device=self.device)
            status = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self._L.twv_tacotron_decoder_grad_backward(g, _ptr(self._blob), _ptr(mem), _ptr(init), _ptr(self.input_lengths), _ptr(dm), _ptr(ws),
                                                                  _ptr(status), _stream(), _ptr(grad), _ptr(d_memory), _ptr(d_init)))
        return grad, d_memory, d_init

    def linear_loss_cotangent(self, linear_targets, loss_coeff=None):
        """d(linear term of add_loss) / d linear_outputs on the last teacher-forced forward_targets pass (tacotron.py:258-282), a
        (N, T_out, num_freq) device tensor: sign(linear - target) * loss_coeff[n] / (N T_out F), with hp.prioritize_loss half of it
        once more over the priority band (reads hp.prioritize_loss, hp.sample_rate, hp.num_freq as add_loss does)."""
        hp = self._hparams
        self._forced_pass("linear_loss_cotangent")
        lin = getattr(self, "linear_outputs", None)
        if lin is None:
            raise ValueError("linear_loss_cotangent needs a forward_targets pass with teacher_forced=True and want_linear=True first")
        N, TO, F = (int(v) for v in lin.shape)
        with torch.cuda.device(self.device):
            co = self._loss_coeff(loss_coeff, N)
            lt = self._device_f32(linear_targets, (N, TO, F), "linear_targets must be %s, got %s")
            out = torch.empty_like(lin)
            _lib.check(self._L.twv_tacotron_linear_loss_grad(_ptr(lin), _ptr(lt), _ptr(co), N, TO, F, 1 if hp.prioritize_loss else 0,
                                                             float(hp.sample_rate), _ptr(out), _stream()))
        return out

    def postnet_grad(self, d_linear, mel=None, mode="inference"):
        """The vector-Jacobian product of the post net (post CBHG + the linear-spectrogram layer): d_linear (N, T_out, num_freq) is the
        cotangent on linear_outputs; mel (N, T_out, num_mels) the post net's input, by default the mel_outputs of the last teacher-forced
        forward_targets pass.  Returns a dict: the gradient of every post_cbhg/* tensor and of the linear layer by name (batch norms as
        (2, C) = d_gamma, d_beta), "d_mel" (the cotangent on mel) and "linear", the recorded forward's output.  mode: a key of BN_MODES;
        "batch" = batch-statistics batch norm over all N * T_out rows (batch_statistics("post") then gives the statistics)."""
        grad, d_mel, lin = self._postnet_grad_blob(d_linear, mel, mode)
        with torch.cuda.device(self.device):
            out = self._named_grads(grad, postnet_grad_layout(self.specs), mode)
        out["d_mel"], out["linear"] = d_mel, lin
        return out

    def _postnet_grad_blob(self, d_linear, mel=None, mode="inference"):
        """postnet_grad's pass with the gradient as the C entry leaves it: (blob-shaped gradient, d_mel, linear)"""
        hp = self._hparams
        mel0, _ = self._forced_pass("postnet_grad")
        if getattr(self, "_blob", None) is None:
            raise ValueError("postnet_grad needs load_weights first")
        with torch.cuda.device(self.device):
            mel = self._device_f32(mel0 if mel is None else mel, None, "")
            N, TO, M = (int(v) for v in mel.shape)
            dl = self._device_f32(d_linear, None, "")
            if M != hp.num_mels or tuple(dl.shape) != (N, TO, hp.num_freq):
                raise ValueError("mel must be (N, T_out, %d) and d_linear (N, T_out, %d), got %s and %s" % (hp.num_mels, hp.num_freq, tuple(mel.shape), tuple(dl.shape)))
            g, ws = self._cbhg_handle("post", (N, TO), mode)
            lin = torch.empty((N, TO, hp.num_freq), dtype=torch.float32, device=self.device)
            grad = torch.empty_like(self._blob)
            d_mel = torch.empty_like(mel)
            status = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self._L.twv_tacotron_postnet_grad_run(g, _ptr(self._blob), _ptr(mel), _ptr(dl), _ptr(ws), _ptr(status), _stream(),
                                                             _ptr(lin), _ptr(grad), _ptr(d_mel)))
        return grad, d_mel, lin

    def encoder_grad(self, d_memory, prenet_masks=None, mode="inference"):
        """The vector-Jacobian product of the encoder (embedding, prenet, encoder CBHG) of the last forward_targets(teacher_forced=True)
        pass: d_memory (N, T_in, 2 * enc_rnn_size) is the cotangent on the encoder output (decoder_grad's "d_memory"); tokens, lengths and,
        for a multi-speaker model, before_highway and the GRUs' initial states are read from that pass.  prenet_masks: None (the evaluation
        graph) or two (N, T_in, enc_prenet_sizes[i]) arrays of multipliers after the prenet's relus.  Returns a dict: the gradient of
        embedding, prenet/* and encoder_cbhg/* by name (batch norms as (2, C) = d_gamma, d_beta), "memory" (the recorded output) and, for a
        multi-speaker model, "d_before_highway" (N, enc_prenet_sizes[1]) and "d_encoder_rnn_init" (N, 2 * enc_rnn_size).  mode: a key of
        BN_MODES; "batch" = batch-statistics batch norm over all N * T_in rows, padded ones included."""
        grad, memory, d_bh, d_init = self._encoder_grad_blob(d_memory, prenet_masks, mode)
        with torch.cuda.device(self.device):
            out = self._named_grads(grad, encoder_grad_layout(self.specs), mode)
        out["memory"] = memory
        if d_bh is not None:
            out["d_before_highway"], out["d_encoder_rnn_init"] = d_bh, d_init
        return out

    def _encoder_grad_blob(self, d_memory, prenet_masks=None, mode="inference"):
        """encoder_grad's pass with the gradient as the C entry leaves it: (blob-shaped gradient, memory, d_before_highway, d_encoder_rnn_init)"""
        hp = self._hparams
        self._forced_pass("encoder_grad")
        if getattr(self, "_blob", None) is None:
            raise ValueError("encoder_grad needs load_weights first")
        N, T = (int(v) for v in self.inputs.shape)
        ENC, P = 2 * hp.enc_rnn_size, hp.enc_prenet_sizes
        with torch.cuda.device(self.device):
            dm = self._device_f32(d_memory, (N, T, ENC), "d_memory must be %s, got %s")
            masks = self._prenet_masks(prenet_masks, (N, T), P)
            bh = init = d_bh = d_init = None
            if self.num_speakers > 1:
                bh, init = self.workspace_view(N, T, "before_highway"), self.workspace_view(N, T, "encoder_rnn_init")
                d_bh = torch.empty((N, P[1]), dtype=torch.float32, device=self.device)
                d_init = torch.empty((N, ENC), dtype=torch.float32, device=self.device)
            g, ws = self._cbhg_handle("encoder", (N, T), mode)
            memory = torch.empty((N, T, ENC), dtype=torch.float32, device=self.device)
            grad = torch.empty_like(self._blob)
            status = torch.zeros(4, dtype=torch.int32, device=self.device)
            _lib.check(self._L.twv_tacotron_encoder_grad_run(g, _ptr(self._blob), _ptr(self.inputs), _ptr(self.input_lengths), _ptr(bh), _ptr(init),
                                                             _ptr(masks[0]), _ptr(masks[1]), _ptr(dm), _ptr(ws), _ptr(status), _stream(),
                                                             _ptr(memory), _ptr(grad), _ptr(d_bh), _ptr(d_init)))
        return grad, memory, d_bh, d_init

    def loss_gradients(self, linear_targets, loss_coeff=None):
        """The gradient of add_loss's `loss` (tacotron.py:258-282) on the last forward_targets(teacher_forced=True) pass, in the evaluation
        graph (inference-mode batch norm, no dropout): linear_loss_cotangent -> postnet_grad -> d_mel = mel_loss_cotangent + the post
        net's d_mel -> decoder_grad -> encoder_grad.  Returns one dict: every checkpoint tensor's gradient by name (batch norms as (2, C) =
        d_gamma, d_beta; the speaker table and its dense layers are not differentiated and absent), "d_init" and, for a multi-speaker
        model, "d_before_highway" and "d_encoder_rnn_init": what the speaker side's gradient starts from."""
        d_linear = self.linear_loss_cotangent(linear_targets, loss_coeff)
        post = self.postnet_grad(d_linear)
        d_mel = self.mel_loss_cotangent(loss_coeff) + post["d_mel"]
        dec = self.decoder_grad(d_mel)
        enc = self.encoder_grad(dec["d_memory"])
        out = {}
        for part in (enc, dec, post):
            out.update({k: v for k, v in part.items() if k not in ("memory", "mel", "linear", "d_mel", "d_memory")})
        return out

    def _speaker_grad_blob(self, d_before_highway, d_encoder_rnn_init, d_init, grad=None):
        """twv_tacotron_speaker_grad on the speaker ids of the last pass: the speaker tensors' ranges of `grad` (a new blob-shaped buffer,
        other ranges unwritten, when None) are written; returns it"""
        hp = self._hparams
        if getattr(self, "_blob", None) is None:
            raise ValueError("speaker_grad needs load_weights first")
        sp = getattr(self, "speaker_id", None)
        if self.num_speakers > 1 and sp is None:
            raise ValueError("speaker_grad needs a pass (infer / forward_targets) first: it reads that pass's speaker ids")
        N = int(sp.shape[0]) if sp is not None else int(np.shape(d_init)[0])
        if sp is None:          # a single-speaker model: the library refuses it in its own words
            sp = torch.zeros(N, dtype=torch.int32, device=self.device)
        ninit = hp.attention_state_size + hp.dec_layer_num * hp.dec_rnn_size
        with torch.cuda.device(self.device):
            d_bh = self._device_f32(d_before_highway, (N, hp.enc_prenet_sizes[1]), "d_before_highway must be %s, got %s")
            d_ei = self._device_f32(d_encoder_rnn_init, (N, 2 * hp.enc_rnn_size), "d_encoder_rnn_init must be %s, got %s")
            d_di = self._device_f32(d_init, (N, ninit), "d_init must be %s, got %s")
            if grad is None:
                grad = torch.empty_like(self._blob)
            need = max(self._L.twv_tacotron_speaker_grad_scratch_bytes(self._h, N) // 4, 4)
            scratch = self.__dict__.get("_speaker_scratch")
            if scratch is None or scratch.numel() < need:
                scratch = self._speaker_scratch = torch.empty(need, dtype=torch.float32, device=self.device)
            _lib.check(self._L.twv_tacotron_speaker_grad(self._h, _ptr(self._blob), _ptr(sp), N, _ptr(d_bh), _ptr(d_ei), _ptr(d_di), _ptr(scratch),
                                                         _ptr(grad), _stream()))
        return grad

    def speaker_grad(self, d_before_highway, d_encoder_rnn_init, d_init):
        """The gradient of the speaker side of a multi-speaker 'deepvoice' model from the three cotangents loss_gradients hands back
        (encoder_grad's "d_before_highway" and "d_encoder_rnn_init", decoder_grad's "d_init"), for the speaker ids of the last pass.
        Returns a dict by checkpoint name: speaker_embedding and dense* kernel / bias, or the five tables of speaker_embedding_size 1
        (tacotron.py:64-84).  A single-speaker model and model_type 'simple' are refused by the library."""
        grad = self._speaker_grad_blob(d_before_highway, d_encoder_rnn_init, d_init)
        return self._named_grads(grad, speaker_grad_layout(self.specs))

    def variable_gradients(self, linear_targets, loss_coeff=None):
        """loss_gradients plus the speaker tensors: the gradient of add_loss's `loss` with respect to every trainable checkpoint tensor of the
        model, in the evaluation graph (moving-average batch norm, no dropout).  Keeps loss_gradients' hand-off entries."""
        out = self.loss_gradients(linear_targets, loss_coeff)
        if self.num_speakers > 1:
            out.update(self.speaker_grad(out["d_before_highway"], out["d_encoder_rnn_init"], out["d_init"]))
        return out

    def add_loss(self, linear_targets, loss_coeff=None):
        """tacotron.py:258-282 on the outputs of the last forward_targets pass: sets `.loss`, `.mel_loss`, `.linear_loss` and
        `.loss_without_coeff` (Python floats) and returns them as a dict.  loss_coeff: one factor per utterance (ones when None,
        datafeeder_tacotron.py:263).  Reads hp.prioritize_loss, hp.sample_rate, hp.num_freq."""
        hp = self._hparams
        if getattr(self, "mel_targets", None) is None or getattr(self, "linear_outputs", None) is None:
            raise ValueError("add_loss needs a forward_targets pass with want_linear=True first")
        mel, lin, tgt = self.mel_outputs, self.linear_outputs, self.mel_targets
        N, TO = int(mel.shape[0]), int(mel.shape[1])
        if tuple(tgt.shape) != tuple(mel.shape) or tuple(lin.shape) != (N, TO, hp.num_freq):
            raise ValueError("outputs %s / %s and mel_targets %s do not belong to one forward_targets pass"
                             % (tuple(mel.shape), tuple(lin.shape), tuple(tgt.shape)))
        with torch.cuda.device(self.device):
            lt = self._device_f32(linear_targets, (N, TO, hp.num_freq), "linear_targets must be %s, got %s")
            co = self._loss_coeff(loss_coeff, N)
            out = torch.empty(4, dtype=torch.float64, device=self.device)
            _lib.check(self._L.twv_tacotron_loss(_ptr(mel), _ptr(lin), _ptr(tgt), _ptr(lt), _ptr(co), N, TO, hp.num_mels, hp.num_freq,
                                                 1 if hp.prioritize_loss else 0, float(hp.sample_rate), _ptr(out), _stream()))
            v = [float(x) for x in out.cpu().numpy()]
        self.linear_targets, self.loss_coeff = lt, co
        self.loss, self.mel_loss, self.linear_loss, self.loss_without_coeff = v
        return {"loss": v[0], "mel_loss": v[1], "linear_loss": v[2], "loss_without_coeff": v[3]}


def __getattr__(name):
    # the reference's Synthesizer (synthesizer.py) has its own module here too; kept importable from this one
    if name == "Synthesizer":
        from .synthesizer import Synthesizer
        return Synthesizer
    raise AttributeError(name)
