"""Host-side mirror of the reference's Tacotron update rule (tacotron/tacotron.py:285-313 `add_optimizer`) over the HIP C-ABI, on the
EVALUATION graph:

    model = Tacotron(hparams, num_speakers); model.load_weights(tensors)
    trainer = TacotronTrainer(model, randomly_initialized=True)
    losses = trainer.step(inputs, input_lengths, speaker_id, mel_targets, linear_targets)     # == sess.run([model.loss, model.optimize])

One step is forward_targets(teacher_forced=True) -> add_loss -> the three gradient passes and the speaker side -> the gradient of the
training vector -> tf.clip_by_global_norm(gradients, 1.0) -> AdamOptimizer(lr, adam_beta1, adam_beta2) -> the new inference blob, all on
the device; the only device -> host traffic is add_loss's four numbers.

That is TacotronTrainer(training=False), the default: the moving statistics are frozen and there is no dropout -- a fine-tuning step with
frozen batch norm.  The moving statistics ride along in the flat Adam call with a zero gradient and zero moments, which leaves them
untouched bit for bit (TensorFlow does not hand non-trainable variables to the optimiser at all).

TacotronTrainer(training=True, seed=s) is the reference's is_training=True graph: batch-statistics batch norm after every
convolution of both CBHGs, dropout 0.5 after both relus of the encoder prenet and of the decoder prenet (masks from a counter-based
generator keyed by (seed, global_step, site): TensorFlow's random stream is not reproduced), and the moving-average update of every moving
mean and variance (momentum 0.99, the biased batch variance) run with the optimiser.  One step is forward_targets(teacher_forced=True) for
the speaker side's values -> the recording forwards of the encoder, the decoder and the post net in that mode -> add_loss on their outputs
-> the three backwards -> the speaker side -> clip -> Adam -> the moving update -> the new inference blob.  The seed is a constructor
argument and is not stored in a checkpoint: restore into a trainer made with the same seed to continue the same mask sequence.

With an initialised torch.distributed process group (or a reduction callable of the caller's) the step is data-parallel: ONE
all-reduce per step over one flat buffer -- the unclipped gradient, a failure flag and, in training mode, both CBHGs' batch statistics --
summed and divided by the world size before the clip; `step(..., failed=True)` and `peer_failure()` are WaveNetTrainer's protocol.
`init_weights(seed)` draws the reference's initial values on the host.  The data feeder and the staging of its batches are
tacotron_feed.py, the command line is train_tacotron.py.
PyTorch is used for device memory, streams and the collective only."""
import os

import numpy as np
import torch

from . import _lib
from . import checkpoint as ckpt
from .tacotron import BN_MOMENTUM, _ptr, _stream, flatten_variables, training_layout
from .train import allreduce_sum_

DROPOUT_RATE = 0.5       # modules.py:15-23 prenet: tf.layers.dropout(rate=0.5, training=is_training)
CLIP_NORM = 1.0          # tacotron.py:306 tf.clip_by_global_norm(gradients, 1.0)
ADAM_EPSILON = 1e-8      # tf.train.AdamOptimizer's default
SCOPE = "model/inference/"


def learning_rate(lr0, step, mode=0, randomly_initialized=True):
    """tacotron.py:292-303 with step = global_step + 1.  mode 0: lr0 * w^0.5 * min(step * w^-1.5, step^-0.5), w = 4000 warm-up steps for a
    randomly initialised model and 40000 otherwise (the peak lr0 is reached at step = w); mode 1: lr0 * 0.95^(step / 3000)"""
    step = float(step)
    if mode == 0:
        w = 4000.0 if randomly_initialized else 40000.0
        return float(lr0) * w ** 0.5 * min(step * w ** -1.5, step ** -0.5)
    if mode == 1:
        return float(lr0) * 0.95 ** (step / 3000.0)
    raise ValueError("decay_learning_rate_mode must be 0 or 1, got %r" % (mode,))


TRUNCATED_VARIANCE = 0.7737413      # the variance of a unit normal cut at two standard deviations: 1 - 4 pdf(2) / (2 cdf(2) - 1)


def _truncated_normal(rng, shape, stddev):
    """tf.truncated_normal_initializer(stddev): normal draws further than two standard deviations from 0 are drawn again"""
    a = rng.standard_normal(int(np.prod(shape)))
    while True:
        far = np.abs(a) > 2.0
        if not far.any():
            return (a * stddev).reshape(shape).astype(np.float32)
        a[far] = rng.standard_normal(int(far.sum()))


def glorot_limit(shape):
    """tf.glorot_uniform_initializer's bound sqrt(6 / (fan_in + fan_out)): a dense kernel (in, out) has fans in and out, a conv1d kernel
    (taps, in, out) taps * in and taps * out, a vector (n) n and n ([RECALLED-TF] init_ops._compute_fans)"""
    shape = tuple(int(v) for v in shape)
    if len(shape) == 1:
        fan_in = fan_out = shape[0]
    else:
        taps = int(np.prod(shape[:-2]))
        fan_in, fan_out = taps * shape[-2], taps * shape[-1]
    return float(np.sqrt(6.0 / (fan_in + fan_out)))


# speaker_embedding_size == 1 (tacotron.py:69-75): the five speaker-dependent vectors are tables made by modules.py:10-12 get_embed
_SPEAKER_TABLES = ("before_highway", "encoder_rnn_init_state", "attention_rnn_init_state", "decoder_rnn_init_states")


def initializer_of(name, shape):
    """(kind, parameter) of a checkpoint tensor's initial value, the reference's tf.global_variables_initializer() by distribution:
      "truncated_normal", stddev   embedding and speaker_embedding 0.5 (tacotron.py:51, :65), the tables of speaker_embedding_size 1 0.1
                                   (modules.py:11)
      "glorot_uniform", limit      every dense, conv1d and GRU kernel, attention_v and loc_sen's attention_variable: tf.layers' and
                                   tf.get_variable's default ([RECALLED-TF]; rnn_wrappers.py:719-721 asks for xavier by name)
      "constant", value            GRU gate biases 1 and candidate biases 0 ([RECALLED-TF] GRUCell's bias_initializer None), highway T biases
                                   -1 (modules.py:88), attention_g sqrt(1 / units) ([RECALLED-TF] _bahdanau_score; Luong's scale 1), attention_b 0,
                                   attention_score_bias score_bias_init = 0 ([RECALLED-TF] BahdanauMonotonicAttention's default; tacotron.py:128-130
                                   does not pass one), every other bias 0
      "batch_normalization", None  gamma 1, beta 0, moving mean 0, moving variance 1 ([RECALLED-TF] tf.layers.batch_normalization)
    alignments_bias (rnn_wrappers.py:566, zeros) belongs to 'bah_mon_norm_hccho', which is not built and has no tensor here."""
    base = name.rsplit("/", 1)[-1]
    if name.endswith("batch_normalization"):
        return "batch_normalization", None
    if name in ("embedding", "speaker_embedding"):
        return "truncated_normal", 0.5
    if "/" not in name and name.startswith(_SPEAKER_TABLES):
        return "truncated_normal", 0.1
    if base == "attention_g":
        return "constant", (1.0 if "luong" in name else None)         # (None: sqrt(1 / units), filled in by initial_tensors)
    if base in ("attention_b", "attention_score_bias", "attention_bias"):
        return "constant", 0.0
    if base in ("attention_v", "attention_variable", "kernel"):
        return "glorot_uniform", glorot_limit(shape)
    if base == "bias":
        if name.endswith("gates/bias"):
            return "constant", 1.0
        if "/highway_" in name and name.endswith("/T/bias"):
            return "constant", -1.0
        return "constant", 0.0
    raise KeyError("no initializer is known for %s" % name)


def initial_tensors(specs, hp, seed=0):
    """{name: float32 array} for every tensor of `specs`, drawn on the host from RandomState(seed) in the order of the specs: the same
    seed gives the same bits on every rank.  By distribution, not by TensorFlow's random stream (initializer_of)."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, shape in specs:
        kind, value = initializer_of(name, shape)
        if kind == "batch_normalization":
            C_ = shape[1]
            out[name] = np.stack([np.ones(C_), np.zeros(C_), np.zeros(C_), np.ones(C_)]).astype(np.float32)
        elif kind == "truncated_normal":
            out[name] = _truncated_normal(rng, shape, value)
        elif kind == "glorot_uniform":
            out[name] = rng.uniform(-value, value, shape).astype(np.float32)
        else:
            if value is None:
                value = np.sqrt(1.0 / hp.attention_size)
            out[name] = np.full(shape, value, np.float32)
    return out


def _copy_runs(specs, picks):
    """[(first float, one past the last)] of the maximal runs of blob floats whose tensor satisfies pick(i, name)"""
    runs, off = [], 0
    for i, (n, shp) in enumerate(specs):
        size = 2 * shp[1] if n.endswith("batch_normalization") else int(np.prod(shp))
        if picks(i, n):
            if runs and runs[-1][1] == off:
                runs[-1][1] = off + size
            else:
                runs.append([off, off + size])
        off += size
    return [tuple(r) for r in runs]


class TacotronTrainer(object):
    def __init__(self, model, randomly_initialized=True, training=False, seed=0, group=None, allreduce=None, attention_gradients=None):
        """model: a Tacotron, with weights loaded or to be given its weights by `restore`; the trainer updates the model's blob in place, so
        `infer` and `forward_targets` see the new weights after every step.  randomly_initialized: tacotron.py:296-299, the warm-up of
        learning-rate mode 0.  training: False = the evaluation graph (frozen batch norm, no dropout), True = the reference's
        is_training=True graph; seed: of the dropout masks (not stored by `save`).  group: the torch.distributed group of a data-parallel
        run (None: the default group, when one is initialised); allreduce: the reduction, `allreduce(flat, group) -> world size` summing
        `flat` in place over the ranks -- train.allreduce_sum_ by default, which without a process group does nothing and returns 1.
        attention_gradients: None leaves the model's setting (Tacotron.attention_gradients, "monotonic" unless the caller changed it);
        "monotonic" or "any" sets it on the model -- "any" trains every attention type the model can be built with, "monotonic" refuses
        all but bah_mon_norm and bah_mon at the first step, and is the model's default only because existing tests pin that."""
        hp = model._hparams
        if attention_gradients is not None:
            model.attention_gradients = attention_gradients
        self.group, self._allreduce = group, (allreduce_sum_ if allreduce is None else allreduce)
        self.model, self.device, self._L = model, model.device, model._L
        self.randomly_initialized = bool(randomly_initialized)
        self.training, self.seed = bool(training), int(seed)
        self.lr0, self.mode = hp.tacotron_initial_learning_rate, hp.decay_learning_rate_mode
        learning_rate(self.lr0, 1, self.mode, self.randomly_initialized)         # (refuses another mode here, not at the first step)
        self.beta1, self.beta2, self.epsilon = hp.adam_beta1, hp.adam_beta2, ADAM_EPSILON
        self.max_checkpoints = getattr(hp, "max_checkpoints", 3)
        self.layout = training_layout(model.specs)
        self.n_variables = int(self._L.twv_tacotron_train_floats(model._h))
        assert self.n_variables == sum(int(np.prod(s)) for _, _, s in self.layout), self.n_variables
        names = [n for n, _ in model.specs]
        first, last = names.index("embedding") + 1, names.index("prenet/dense_1/kernel")
        dec0, dec1 = names.index("memory_layer/kernel"), names.index("decoder/output_projection_wrapper/bias")
        # each of the three gradient passes zeroes the whole blob-shaped buffer it is given before it writes its own range (tgrad::Handle::
        # begin), so one buffer cannot serve all three: each writes a buffer of its own and its range is copied into the step's gradient
        self._runs = {"encoder": _copy_runs(model.specs, lambda i, n: not first <= i < last and i < dec0),
                      "decoder": _copy_runs(model.specs, lambda i, n: dec0 <= i <= dec1),
                      "post": _copy_runs(model.specs, lambda i, n: i > dec1)}
        self._speaker = model.num_speakers > 1
        self.global_step = 0
        self.vars = None
        if getattr(model, "_blob", None) is not None:
            self._set_variables(self._model_tensors())

    # ---- variables
    def _model_tensors(self):
        """the checkpoint tensors the model holds: the blob's ranges, and the raw (4, C) tensors load_weights kept of every batch norm"""
        m = self.model
        blob, out, off = m._blob.cpu().numpy(), {}, 0
        for n, shp in m.specs:
            if n.endswith("batch_normalization"):
                out[n] = np.asarray(m._bn_raw[n], np.float32)
                off += 2 * shp[1]
            else:
                size = int(np.prod(shp))
                out[n] = blob[off:off + size].reshape(shp).copy()
                off += size
        return out

    def _set_variables(self, tensors, m=None, v=None):
        flat = flatten_variables(self.model.specs, tensors)
        assert flat.size == self.n_variables, (flat.size, self.n_variables)
        with torch.cuda.device(self.device):
            self.vars = torch.from_numpy(flat).to(self.device)
            self.model._train_vec = self.vars               # (batch-mode passes read gamma and beta from the vector the steps update)
            self.m = torch.zeros_like(self.vars) if m is None else torch.from_numpy(m).to(self.device)
            self.v = torch.zeros_like(self.vars) if v is None else torch.from_numpy(v).to(self.device)
            self._shadow = self.vars.clone()                # twv_adam_ema_step's shadow: written, never read
            # the step's reduction buffer: the gradient, then ONE word for the failure flag, then (from the next multiple of four floats) both
            # CBHGs' batch statistics, encoder first -- one all-reduce carries all three
            self._stat_floats = [sum(2 * shp[1] for n, shp in self.model.specs if n.startswith(scope) and n.endswith("batch_normalization"))
                                 for scope in ("encoder_cbhg/", "post_cbhg/")]
            self._stats_at = (self.n_variables + 1 + 3) // 4 * 4
            self._gbuf = torch.zeros(self._stats_at + sum(self._stat_floats), dtype=torch.float32, device=self.device)
            self.grads = self._gbuf[:self.n_variables]
            self._flag = self._gbuf[self.n_variables:self.n_variables + 1]
            self._gblob = torch.zeros_like(self.model._blob)
            self._clip_scratch = torch.empty(self.n_variables + 2048, dtype=torch.float32, device=self.device)

    def _named(self, flat):
        host = flat.detach().cpu().numpy()
        return {n: host[off:off + int(np.prod(shp))].reshape(shp).copy() for n, off, shp in self.layout}

    def variables(self):
        """every checkpoint tensor by tacotron_specs name (batch norms as (4, C)), numpy"""
        return self._named(self.vars)

    def gradients(self):
        """the last step's gradient of the training vector as Adam saw it (after the clip), by name"""
        return self._named(self.grads)

    def learning_rate(self, step):
        """the schedule at step = global_step + 1 (tacotron.py:292-303)"""
        return learning_rate(self.lr0, step, self.mode, self.randomly_initialized)

    # ---- compute_gradients
    def loss_and_gradients(self, inputs, input_lengths, speaker_id, mel_targets, linear_targets, loss_coeff=None):
        """forward_targets(teacher_forced=True), add_loss and d loss / d (training vector) into self.grads (unclipped); returns add_loss's dict"""
        m = self.model
        if self.vars is None:
            raise RuntimeError("no weights: give the model its weights (load_weights) before the trainer is made, or call restore")
        if self.training:
            return self._training_loss_and_gradients(inputs, input_lengths, speaker_id, mel_targets, linear_targets, loss_coeff)
        m.forward_targets(inputs, input_lengths, speaker_id, mel_targets, teacher_forced=True)
        out = m.add_loss(linear_targets, loss_coeff)
        self._forward_done()
        with torch.cuda.device(self.device):
            g = self._gblob
            post, d_mel_post, _ = m._postnet_grad_blob(m.linear_loss_cotangent(linear_targets, loss_coeff))
            self._collect(g, post, "post")
            dec, d_memory, d_init, _ = m._decoder_grad_blob(m.mel_loss_cotangent(loss_coeff) + d_mel_post)
            self._collect(g, dec, "decoder")
            enc, _, d_bh, d_ei = m._encoder_grad_blob(d_memory)
            self._collect(g, enc, "encoder")
            self._passes_done()
            if self._speaker:
                m._speaker_grad_blob(d_bh, d_ei, d_init, grad=g)
            self._speaker_done()
            _lib.check(self._L.twv_tacotron_grad_convert(m._h, _ptr(self.vars), _ptr(g), _ptr(self.grads), _stream()))
        return out

    def dropout_masks(self, N, T, steps, step=None):
        """the four masks of a step (global_step by default): encoder prenet 1, 2 (N, T, enc_prenet_sizes[i]), decoder prenet 1, 2
        (N, steps, dec_prenet_sizes[i])"""
        hp, m = self.model._hparams, self.model
        step = self.global_step if step is None else int(step)
        shapes = [(N, T, hp.enc_prenet_sizes[0]), (N, T, hp.enc_prenet_sizes[1]), (N, steps, hp.dec_prenet_sizes[0]), (N, steps, hp.dec_prenet_sizes[1])]
        return [m.dropout_mask(shp, self.seed, step, site, DROPOUT_RATE) for site, shp in enumerate(shapes)]

    def _training_loss_and_gradients(self, inputs, input_lengths, speaker_id, mel_targets, linear_targets, loss_coeff):
        """the training-mode chain: every recording forward before any backward, add_loss on the training-mode outputs"""
        m = self.model
        # the speaker side's values (before_highway, the GRUs' and the decoder's initial states: no batch norm, no dropout in them), the
        # tokens and the targets on the device
        m.forward_targets(inputs, input_lengths, speaker_id, mel_targets, teacher_forced=True)
        N, T = (int(v) for v in m.inputs.shape)
        steps = int(m.mel_targets.shape[1]) // m._hparams.reduction_factor
        with torch.cuda.device(self.device):
            masks = self.last_masks = self.dropout_masks(N, T, steps)
            memory = m.encoder_grad_forward(masks[:2], mode="batch")
            mel = m.decoder_grad_forward(memory, masks[2:])
            lin = m.postnet_grad_forward(mel, mode="batch")
            m.mel_outputs, m.linear_outputs = mel, lin       # (add_loss and the two loss cotangents read the pass's outputs from here)
            out = m.add_loss(linear_targets, loss_coeff)
            self._forward_done()
            g = self._gblob
            post, d_mel_post = m.postnet_grad_backward(m.linear_loss_cotangent(linear_targets, loss_coeff))
            self._collect(g, post, "post")
            dec, d_memory, d_init = m.decoder_grad_backward(m.mel_loss_cotangent(loss_coeff) + d_mel_post)
            self._collect(g, dec, "decoder")
            enc, d_bh, d_ei = m.encoder_grad_backward(d_memory)
            self._collect(g, enc, "encoder")
            self._passes_done()
            if self._speaker:
                m._speaker_grad_blob(d_bh, d_ei, d_init, grad=g)
            self._speaker_done()
            _lib.check(self._L.twv_tacotron_grad_convert_batch(m._h, _ptr(g), _ptr(self.grads), _stream()))
            self._stats = (m._batch_stats_flat("encoder"), m._batch_stats_flat("post"))
        return out

    def _collect(self, grad, part, which):
        for a, b in self._runs[which]:
            grad[a:b].copy_(part[a:b])

    # (phase boundaries: scripts/tacotron_train_bench.py records events here)
    def _forward_done(self):
        pass

    def _passes_done(self):
        pass

    def _speaker_done(self):
        pass

    # ---- clip_by_global_norm + apply_gradients
    def apply_gradients(self):
        m = self.model
        lr = self.learning_rate(self.global_step + 1)
        with torch.cuda.device(self.device):
            _lib.check(self._L.twv_clip_by_global_norm(_ptr(self.grads), self.n_variables, 1.0, CLIP_NORM, _ptr(self._clip_scratch), _stream()))
            _lib.check(self._L.twv_adam_ema_step(_ptr(self.vars), _ptr(self.grads), _ptr(self.m), _ptr(self.v), _ptr(self._shadow),
                                                self.n_variables, lr, self.beta1, self.beta2, self.epsilon, self.global_step + 1, 0.0, 1.0,
                                                _stream()))
            if self.training:
                # tacotron.py:310-313: the moving-average updates run with the optimiser.  Adam leaves the moving slots bit for bit, so the
                # order of the two is free
                _lib.check(self._L.twv_tacotron_moving_update(m._h, _ptr(self.vars), _ptr(self._stats[0]), _ptr(self._stats[1]), BN_MOMENTUM, _stream()))
            self._refold()
            if self.training:
                self._refresh_bn_raw()
        self.global_step += 1
        return lr

    def _refold(self):
        """the training vector -> the model's blob and packed weights (the moving statistics never move, so the mean and variance the model
        keeps on the host for bn_grad_from_inference_pair stay those of the blob)"""
        m = self.model
        _lib.check(self._L.twv_tacotron_refold(m._h, _ptr(self.vars), _ptr(m._blob), _stream()))
        _lib.check(self._L.twv_tacotron_pack(m._h, _ptr(m._blob), _ptr(m._packed), _stream()))

    def _refresh_bn_raw(self):
        """after a training-mode step the moving statistics have moved: the (4, C) tensors the model keeps on the host for
        bn_grad_from_inference_pair (loss_gradients on the evaluation graph) are read back from the training vector"""
        m = self.model
        bns = [(n, off, shp) for n, off, shp in self.layout if n.endswith("batch_normalization")]
        host = torch.cat([self.vars[off:off + int(np.prod(shp))] for _, off, shp in bns]).cpu().numpy().astype(np.float64)      # (one copy)
        at = 0
        for n, _, shp in bns:
            size = int(np.prod(shp))
            m._bn_raw[n] = host[at:at + size].reshape(shp).copy()
            at += size

    def step(self, inputs, input_lengths, speaker_id, mel_targets, linear_targets, loss_coeff=None, failed=False):
        """one sess.run([model.loss, model.optimize]) on the evaluation graph (training=False) or the training graph (training=True); returns add_loss's dict (the loss BEFORE the update) and
        advances global_step.  `last_learning_rate` is the rate the update used.

        Data-parallel (a process group, or the constructor's `allreduce`): the unclipped gradient, the failure flag and, in training
        mode, both CBHGs' batch statistics are summed over the ranks in ONE all-reduce and divided by the world size before the clip.
        Each rank has normalised its batch norms with its own statistics, as a tower would; the moving averages move by the ranks' MEAN
        statistics, so the variables stay identical on every rank (the reference has one GPU: this is an extension).
        failed=True: this rank has no batch; it joins the collective with zeros and the flag set, applies nothing and returns None.  A
        rank whose loss / gradient computation raises joins the same way before re-raising.  NO rank applies a step whose reduction
        carries a failed rank: with more than one rank the flag is read (one host sync) before the clip, Adam and global_step move.
        With one rank the reduction does nothing and nothing is divided: the step is the single-device step bit for bit."""
        err, out = None, None
        if not failed:
            self._flag.zero_()
            try:
                out = self.loss_and_gradients(inputs, input_lengths, speaker_id, mel_targets, linear_targets, loss_coeff)
                if self.training:
                    at = self._stats_at
                    for part in self._stats:
                        self._gbuf[at:at + part.numel()].copy_(part)
                        at += part.numel()
            except Exception as e:                     # noqa: BLE001 -- re-raised below, after the peers have been released
                err, failed = e, True
        if failed:
            self._gbuf.zero_()
            self._flag.fill_(1.0)
        world = self._allreduce(self._gbuf, self.group)
        if err is not None:
            raise err
        if world > 1:
            self._gbuf.div_(world)
            if self.training and not failed:
                a, b = self._stats_at, self._stats_at + self._stat_floats[0]
                self._stats = (self._gbuf[a:b].clone(), self._gbuf[b:b + self._stat_floats[1]].clone())
        if not failed and (world == 1 or not self.peer_failure()):
            self.last_learning_rate = self.apply_gradients()
        return out

    def peer_failure(self):
        """True when some rank joined the last step's all-reduce with failed=True (host sync)"""
        return bool(float(self._flag.item()) > 0.0)

    # ---- tf.global_variables_initializer
    def init_weights(self, seed=0):
        """the reference's initial values (initial_tensors: by distribution, drawn on the host from `seed`, identical on every rank) into
        the model and the trainer; the optimiser's moments and global_step start from zero.  Returns the tensors."""
        tensors = initial_tensors(self.model.specs, self.model._hparams, seed)
        self.model.load_weights(tensors)
        self._set_variables(tensors)
        self.global_step = 0
        return tensors

    # ---- saver.save / restore
    def save(self, logdir, step=None, include_optimizer=True, max_to_keep=None):
        """writes `logdir/model.ckpt-<step>` as a TensorFlow V2 bundle + the `checkpoint` state file: the variables under
        'model/inference/' (checkpoint.tacotron_variables; Synthesizer.load reads them), `global_step`, and with include_optimizer the Adam
        moments of the trainable variables under `optimizer/<variable>/Adam`, `/Adam_1` and `optimizer/beta{1,2}_power` ([RECALLED-TF] slot
        naming, unverified, as WaveNetTrainer.save)."""
        step = self.global_step if step is None else int(step)
        var = ckpt.tacotron_variables(self.variables(), SCOPE)
        var["global_step"] = np.asarray(step, np.int32)
        if include_optimizer:
            for suffix, flat in (("/Adam", self.m), ("/Adam_1", self.v)):
                for k, a in ckpt.tacotron_variables(self._named(flat), SCOPE).items():
                    if not k.endswith(("/moving_mean", "/moving_variance")):         # (not trainable: no slots)
                        var["optimizer/" + k + suffix] = a
            var["optimizer/beta1_power"] = np.asarray(self.beta1 ** (self.global_step + 1), np.float32)
            var["optimizer/beta2_power"] = np.asarray(self.beta2 ** (self.global_step + 1), np.float32)
        prefix = os.path.join(logdir, "model.ckpt-%d" % step)
        ckpt.write_bundle(prefix, var)
        if max_to_keep is None:
            max_to_keep = self.max_checkpoints
        kept = [q for q in ckpt.all_checkpoint_paths(logdir) if q != prefix and os.path.exists(q + ".index")] + [prefix]
        while max_to_keep and len(kept) > max_to_keep:
            ckpt.delete_bundle(kept.pop(0))
        ckpt.write_checkpoint_state(logdir, prefix, kept)
        return prefix

    def restore(self, path, verify=False):
        """logdir or bundle prefix -> global step.  The variables are required and go into the model too (load_weights); the Adam moments
        are taken when the bundle has them all (else zeros, a fresh optimizer)."""
        prefix = ckpt.resolve(path)
        var = ckpt.read_bundle(prefix, verify=verify)
        specs = self.model.specs
        tensors = ckpt.tacotron_tensors(var, specs, SCOPE)
        self.model.load_weights(tensors)

        def slots(suffix):
            got = {}
            for k in ckpt.tacotron_variables(tensors, SCOPE):
                if k.endswith(("/moving_mean", "/moving_variance")):
                    got[k] = np.zeros_like(var[k], dtype=np.float32)
                elif "optimizer/" + k + suffix in var:
                    got[k] = var["optimizer/" + k + suffix]
                else:
                    return None
            return flatten_variables(specs, ckpt.tacotron_tensors(got, specs, SCOPE))
        m, v = slots("/Adam"), slots("/Adam_1")
        if m is None or v is None:
            m = v = None
        self._set_variables(tensors, m, v)
        self.global_step = int(var["global_step"]) if "global_step" in var else ckpt.checkpoint_step(prefix)
        return self.global_step
