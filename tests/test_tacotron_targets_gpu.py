"""-m gpu: Tacotron passes with mel targets (twv_tacotron_forward_targets: TacoTrainingHelper's step count, free-running and teacher-forced)
on every decoder route, against twv_tacotron_infer bit for bit and against the float64 restatement tests/torch_tacotron_targets_ref.py; and
the evaluation losses (twv_tacotron_loss) against its numpy float64 add_loss.

Small geometry (that of tests/test_attention_types_gpu.py, decoder widths at their defaults so that the resident kernel qualifies):
max_iters = 8, r = 5, 5 steps (t_out = 25) unless stated.  Every pass is computed once per route and shared between the tests."""
import functools

import numpy as np
import pytest

from helpers import first_mismatch

pytestmark = pytest.mark.gpu

# float32 kernel vs float64 restatement, max |kernel - restatement| / max |restatement| per output: the project's bar for the decoder
# (tests/test_attention_types_gpu.py RTOL).  Measured distances: profiles/tacotron_targets_parity.txt.
RTOL = 5e-5
R, STEPS, T_OUT, MAX_ITERS = 5, 5, 25, 8
SMALL = dict(enc_bank_size=4, post_bank_size=3, num_freq=129)
BATCHES = {3: (19, [19, 12, 7]), 9: (23, [23, 20, 17, 14, 11, 8, 5, 23, 2]), 17: (23, [23 - i for i in range(17)])}
# route -> (hparams overrides, num_speakers, decoder_groups, batch, kernel)
ROUTES = {
    "resident-3": ({}, 2, 0, 3, "tc_decoder_x_kernel"),
    "resident-9": ({}, 2, 0, 9, "tc_decoder_x_kernel"),                 # two utterances on one XCD
    "resident-17": ({}, 2, 0, 17, "tc_decoder_x_kernel"),               # three per XCD: the matrix-core instantiation
    "split-1": ({}, 2, 1, 3, "tc_decoder_g_kernel"),
    "split-4": ({}, 2, 4, 3, "tc_decoder_g_kernel"),
    "split-8": ({}, 2, 8, 3, "tc_decoder_g_kernel"),
    "single": ({}, 2, -1, 3, "tc_decoder_kernel"),
    "split-bah_norm": (dict(attention_type="bah_norm"), 2, 4, 3, "tc_decoder_g_kernel"),
    "split-loc_sen": (dict(attention_type="loc_sen"), 2, 4, 3, "tc_decoder_g_kernel"),
    "simple": (dict(model_type="simple"), 4, 4, 3, "tc_decoder_g_kernel"),
    "single-speaker": ({}, 1, 0, 3, "tc_decoder_x_kernel"),
}
ALL = sorted(ROUTES)
ONE_PER_KERNEL = ["resident-3", "split-4", "single"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _hp(**kw):
    import twvk_amd
    hp = twvk_amd.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _tokens(N, T, lengths, seed):
    rng = np.random.RandomState(seed)
    tok = rng.randint(2, 80, (N, T)).astype(np.int32)
    for n, ln in enumerate(lengths):
        tok[n, ln - 1] = 1                      # EOS
        tok[n, ln:] = 0                         # pad
    return tok, np.asarray(lengths, np.int32)


def _np(outs):
    return [x.cpu().numpy() for x in outs]


def _same(a, b, what):
    for name, x, y in zip(("mel", "linear", "alignments"), a, b):
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        assert np.isfinite(x).all() and np.isfinite(y).all(), (what, name)
        assert first_mismatch(x, y) is None, (what, name, first_mismatch(x, y))


class _Route(object):
    """a route's model on the max_iters = 8 handle, its inputs, and its passes (each computed once)"""

    def __init__(self, name):
        import torch_attention_ref as AR
        from twvk_amd.tacotron import Tacotron
        kw, self.num_speakers, self.groups, self.N, self.kernel = ROUTES[name]
        self.name, self.kw = name, kw
        self.hp = _hp(max_iters=MAX_ITERS, **dict(SMALL, **kw))
        self.m = Tacotron(self.hp, num_speakers=self.num_speakers)
        self.w = AR.random_tensors(self.m.specs, seed=131)
        self.m.load_weights(self.w)
        self.m.set_option("decoder_groups", self.groups)
        self.T, lengths = BATCHES[self.N]
        self.tok, self.ln = _tokens(self.N, self.T, lengths, 132)
        self.spk = (np.arange(self.N) % self.num_speakers).astype(np.int32)
        assert self.m.decoder_kernel_name(self.N, self.T) == self.kernel, (name, self.m.decoder_kernel_name(self.N, self.T))
        self._passes = {}

    def other_handle(self, max_iters):
        """a second handle with the same weights and options and another max_iters"""
        from twvk_amd.tacotron import Tacotron
        m = Tacotron(_hp(max_iters=max_iters, **dict(SMALL, **self.kw)), num_speakers=self.num_speakers)
        m.load_weights(self.w)
        m.set_option("decoder_groups", self.groups)
        assert m.decoder_kernel_name(self.N, self.T) == self.kernel
        return m

    def forward(self, targets, teacher_forced, t_out=T_OUT):
        if targets is None:
            targets = np.zeros((self.N, t_out, self.hp.num_mels), np.float32)
        return _np(self.m.forward_targets(self.tok, self.ln, self.spk, targets, teacher_forced=teacher_forced))

    def free(self):
        """the free-running pass of 5 steps on the max_iters = 8 handle"""
        if "free" not in self._passes:
            self._passes["free"] = self.forward(None, False)
        return self._passes["free"]

    def random_targets(self):
        """finite targets in the normalised mel range (symmetric_mels, max_abs_value = 4)"""
        return np.random.RandomState(133).uniform(-4.0, 4.0, (self.N, T_OUT, self.hp.num_mels)).astype(np.float32)

    def forced(self):
        """the teacher-forced pass on random_targets()"""
        if "forced" not in self._passes:
            self._passes["forced"] = self.forward(self.random_targets(), True)
        return self._passes["forced"]


@functools.lru_cache(maxsize=None)
def _route(name):
    return _Route(name)


# ------------------------------------------------------------------------------------------------ 1. free-running equals infer
@pytest.mark.parametrize("route", ALL)
def test_free_running_equals_infer(torch_cuda, route):
    r = _route(route)
    out = r.free()
    assert out[0].shape == (r.N, T_OUT, 80) and out[1].shape == (r.N, T_OUT, 129) and out[2].shape == (r.N, r.T, STEPS)
    _same(out, _np(r.other_handle(STEPS).infer(r.tok, r.ln, r.spk)), "5 steps on the max_iters=8 handle vs infer on a max_iters=5 handle")
    full = r.forward(None, False, t_out=MAX_ITERS * R)
    _same(full, _np(r.m.infer(r.tok, r.ln, r.spk)), "8 steps vs infer on the same handle")


def test_free_running_takes_a_null_target_buffer(torch_cuda):
    """teacher_forced = 0 uses mel_targets for nothing but the length: NULL is accepted and gives the same pass"""
    import ctypes as C
    from twvk_amd import _lib
    from twvk_amd.tacotron import _ptr, _stream
    torch = torch_cuda
    r = _route("resident-3")
    free = r.free()                                                  # (sizes the model's workspace, sets .inputs / .input_lengths / .speaker_id)
    m = r.m
    mel = torch.empty((r.N, T_OUT, 80), dtype=torch.float32, device="cuda")
    lin = torch.empty((r.N, T_OUT, 129), dtype=torch.float32, device="cuda")
    al = torch.empty((r.N, r.T, STEPS), dtype=torch.float32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    m.forward_targets(r.tok, r.ln, r.spk, np.zeros((r.N, T_OUT, 80), np.float32))
    _lib.check(m._L.twv_tacotron_forward_targets(m._h, _ptr(m._packed), _ptr(m.inputs), _ptr(m.input_lengths), _ptr(m.speaker_id), r.N, r.T,
                                                 None, T_OUT, 0, _ptr(m._ws), _ptr(mel), _ptr(lin), _ptr(al), _ptr(status), _stream()))
    _same(_np((mel, lin, al)), free, "NULL targets, free-running")


# ------------------------------------------------------------------------------------------------ 2. teacher forcing fed its own outputs
@pytest.mark.parametrize("route", ALL)
def test_teacher_forcing_fed_the_free_running_frames(torch_cuda, route):
    """targets whose rows r-1::r are the free-running pass's rows and whose other rows are NaN: the same bits -- the row index is right and
    no other target row is read"""
    r = _route(route)
    free = r.free()
    targets = np.full((r.N, T_OUT, 80), np.nan, np.float32)
    targets[:, R - 1::R] = free[0][:, R - 1::R]
    _same(r.forward(targets, True), free, "teacher-forced on the free-running frames")


# ------------------------------------------------------------------------------------------------ 3. causality of the feed
@pytest.mark.parametrize("route", ONE_PER_KERNEL)
def test_a_target_row_reaches_the_next_step_only(torch_cuda, route):
    r = _route(route)
    base = r.forced()
    assert all(np.isfinite(x).all() for x in base)
    k = 2
    t = r.random_targets()
    t[:, k * R - 1] += 0.75
    out = r.forward(t, True)
    assert first_mismatch(out[0][:, :k * R], base[0][:, :k * R]) is None                    # mel steps 0 .. k-1
    assert first_mismatch(out[2][:, :, :k], base[2][:, :, :k]) is None                      # and their alignment columns
    for n in range(r.N):
        assert np.any(out[0][n, k * R:(k + 1) * R] != base[0][n, k * R:(k + 1) * R]), n    # step k differs
    t = r.random_targets()
    t[:, T_OUT - 1] += 0.75                                                                 # the last row feeds no step
    _same(r.forward(t, True), base, "last target row changed")
    # teacher forcing does change the pass (the free-running pass is another one)
    assert np.any(base[0][:, R:] != r.free()[0][:, R:])
    assert first_mismatch(base[0][:, :R], r.free()[0][:, :R]) is None                       # step 0: the go-frame in both


@pytest.mark.parametrize("route", ONE_PER_KERNEL)
def test_the_last_target_row_is_not_read(torch_cuda, route):
    """row t_out - 1 would feed a step after the last: with NaN there the pass is the same bits, so the kernels do not load it"""
    r = _route(route)
    t = r.random_targets()
    t[:, T_OUT - 1] = np.nan
    _same(r.forward(t, True), r.forced(), "last target row NaN")


# ------------------------------------------------------------------------------------------------ 4. against the float64 restatement
def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def _check_restatement(label, hp, num_speakers, w, tok, ln, spk, attention_type, targets, out):
    import torch_attention_ref as AR
    import torch_tacotron_targets_ref as TR
    ref = TR.forward_targets(w, AR.Dims(hp, num_speakers), tok, ln, spk, attention_type, targets, targets.shape[1], True)
    d = tuple(_rel(a, b) for a, b in zip(out, ref))
    print("%s teacher-forced N=%d T=%d steps=%d: rel distance mel %.2e linear %.2e alignments %.2e"
          % ((label,) + tok.shape + (targets.shape[1] // hp.reduction_factor,) + d))
    assert max(d) <= RTOL, (label, d)


@pytest.mark.parametrize("route", ["resident-3", "resident-17", "split-4", "single", "split-bah_norm", "split-loc_sen", "simple"])
def test_teacher_forced_against_the_restatement(torch_cuda, route):
    r = _route(route)
    _check_restatement(route, r.hp, r.num_speakers, r.w, r.tok, r.ln, r.spk, r.hp.attention_type, r.random_targets(), r.forced())


@pytest.mark.parametrize("attention_type", ["bah_mon", "bah", "luong", "luong_scaled"])
def test_teacher_forced_other_attention_types_against_the_restatement(torch_cuda, attention_type):
    import torch_attention_ref as AR
    from twvk_amd.tacotron import Tacotron
    hp = _hp(max_iters=MAX_ITERS, attention_type=attention_type, **SMALL)
    m = Tacotron(hp, num_speakers=2)
    w = AR.random_tensors(m.specs, seed=141)
    m.load_weights(w)
    T, lengths = BATCHES[3]
    tok, ln = _tokens(3, T, lengths, 142)
    spk = np.array([1, 0, 1], np.int32)
    assert m.decoder_kernel_name(3, T) == "tc_decoder_g_kernel"
    targets = np.random.RandomState(143).uniform(-4.0, 4.0, (3, T_OUT, 80)).astype(np.float32)
    out = _np(m.forward_targets(tok, ln, spk, targets, teacher_forced=True))
    _check_restatement(attention_type, hp, 2, w, tok, ln, spk, attention_type, targets, out)


def test_teacher_forced_default_geometry_25_steps(torch_cuda):
    """the hparams-default model (max_iters = 200, the resident kernel's folded instantiation), 25 of its 200 steps"""
    import torch_attention_ref as AR
    from twvk_amd.tacotron import Tacotron
    hp = _hp()
    m = Tacotron(hp, num_speakers=2)
    w = AR.random_tensors(m.specs, seed=151)
    m.load_weights(w)
    tok, ln = _tokens(3, 40, [40, 29, 13], 152)
    spk = np.array([1, 0, 1], np.int32)
    assert m.decoder_kernel_name(3, 40) == "tc_decoder_x_kernel"
    targets = np.random.RandomState(153).uniform(-4.0, 4.0, (3, 125, 80)).astype(np.float32)
    out = _np(m.forward_targets(tok, ln, spk, targets, teacher_forced=True))
    assert out[0].shape == (3, 125, 80) and out[1].shape == (3, 125, hp.num_freq) and out[2].shape == (3, 40, 25)
    _check_restatement("default geometry", hp, 2, w, tok, ln, spk, "bah_mon_norm", targets, out)


# ------------------------------------------------------------------------------------------------ 5. placement
def test_permuting_the_batch_permutes_the_outputs(torch_cuda):
    r = _route("resident-9")
    base = r.forced()
    perm = np.random.RandomState(161).permutation(r.N)
    assert np.any(perm != np.arange(r.N))
    out = _np(r.m.forward_targets(r.tok[perm], r.ln[perm], r.spk[perm], r.random_targets()[perm], teacher_forced=True))
    _same(out, [x[perm] for x in base], "permuted batch")


# ------------------------------------------------------------------------------------------------ 6. loss
def _loss_case(num_freq, t_out=25, seed=171):
    rng = np.random.RandomState(seed + num_freq + t_out)
    shape_m, shape_l = (3, t_out, 80), (3, t_out, num_freq)
    return [rng.uniform(-4.0, 4.0, s).astype(np.float32) for s in (shape_m, shape_l, shape_m, shape_l)]


def _kernel_loss(torch, arrays, coeff, prioritize, sample_rate):
    import ctypes as C
    from twvk_amd import _lib
    L = _lib.lib()
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    co = torch.from_numpy(np.asarray(coeff, np.float32)).cuda()
    out = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    B, t_out, F = arrays[1].shape
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(L.twv_tacotron_loss(p(dev[0]), p(dev[1]), p(dev[2]), p(dev[3]), p(co), B, t_out, arrays[0].shape[2], F, int(prioritize),
                                   float(sample_rate), p(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out.cpu().numpy()


# (B x t_out x num_freq = 3 x 25 x 129 / 1025 and 3 x 7 x 1025: rows of 129 and 1025 bins are no multiple of a wave's 64 lanes or of its
# 256-element strides, 3 x 7 x 80 mel values are no multiple of the 1024-value mel unit: the tails of both loops)
@pytest.mark.parametrize("num_freq, t_out", [(129, 25), (1025, 25), (1025, 7)])
@pytest.mark.parametrize("prioritize", [False, True])
def test_loss_against_the_restatement(torch_cuda, num_freq, t_out, prioritize):
    import torch_tacotron_targets_ref as TR
    mel, lin, mel_t, lin_t = arrays = _loss_case(num_freq, t_out)
    coeff = [1.0, 0.5, 2.0]
    got = _kernel_loss(torch_cuda, arrays, coeff, prioritize, 24000)
    want = TR.add_loss(mel, lin, mel_t, lin_t, coeff, prioritize, 24000, num_freq)
    rel = [abs(g - w) / abs(w) for g, w in zip(got, want)]
    print("loss F=%d t_out=%d prioritize=%d: kernel %r restatement %r rel %r" % (num_freq, t_out, prioritize, list(got), want, rel))
    assert max(rel) <= 1e-12, (got, want, rel)
    again = _kernel_loss(torch_cuda, arrays, coeff, prioritize, 24000)
    assert got.tobytes() == again.tobytes()                          # two calls: equal bits
    if prioritize:                                                   # the band matters and the coefficients matter
        assert got[2] != TR.add_loss(mel, lin, mel_t, lin_t, coeff, False, 24000, num_freq)[2]
    assert got[0] != got[3]


def test_add_loss_after_forward_targets(torch_cuda):
    r = _route("resident-3")
    rng = np.random.RandomState(181)
    lin_t = rng.uniform(-4.0, 4.0, (r.N, T_OUT, 129)).astype(np.float32)
    coeff = [1.0, 0.5, 2.0]
    mel, lin, _ = r.m.forward_targets(r.tok, r.ln, r.spk, r.random_targets(), teacher_forced=True)
    for prioritize in (False, True):
        r.m._hparams.prioritize_loss = prioritize
        try:
            d = r.m.add_loss(lin_t, coeff)
        finally:
            r.m._hparams.prioritize_loss = False
        got = _kernel_loss(torch_cuda, [mel.cpu().numpy(), lin.cpu().numpy(), r.random_targets(), lin_t], coeff, prioritize, r.hp.sample_rate)
        assert [d["loss"], d["mel_loss"], d["linear_loss"], d["loss_without_coeff"]] == list(got)
        assert (r.m.loss, r.m.mel_loss, r.m.linear_loss, r.m.loss_without_coeff) == tuple(got)
        assert all(isinstance(v, float) and np.isfinite(v) for v in d.values())
    ones = r.m.add_loss(lin_t)                                       # loss_coeff None: ones -> loss == loss_without_coeff's terms
    assert abs(ones["loss"] - ones["loss_without_coeff"]) <= 1e-12 * ones["loss"]


def test_add_loss_after_infer_is_refused(torch_cuda):
    """infer overwrites the outputs of a pass with targets: the targets of that pass must not be paired with them"""
    from twvk_amd.tacotron import Tacotron
    r = _route("split-4")
    m = Tacotron(r.hp, num_speakers=r.num_speakers)
    m.load_weights(r.w)
    m.forward_targets(r.tok, r.ln, r.spk, r.random_targets(), teacher_forced=True)
    assert m.mel_targets is not None
    m.infer(r.tok, r.ln, r.spk)
    assert m.mel_targets is None
    with pytest.raises(ValueError, match="forward_targets pass"):
        m.add_loss(np.zeros((r.N, MAX_ITERS * R, 129), np.float32))
