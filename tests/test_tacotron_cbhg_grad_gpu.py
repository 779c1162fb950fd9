"""-m gpu: the Tacotron encoder and post-net gradients (twv_tacotron_encoder_grad_run / twv_tacotron_postnet_grad_run /
twv_tacotron_linear_loss_grad, Tacotron.encoder_grad / postnet_grad / linear_loss_cotangent / loss_gradients) against the float64 autograd
checker tests/torch_tacotron_cbhg_grad_ref.py under the project's gradient bar (tests/train_cases.py RATIO / FLOOR: per tensor at most 8 x the
float32 autograd run's own distance from float64, floor 5e-6 of the tensor's maximum), and the exact properties of the pass: linearity in
the cotangent, per-utterance independence, repeatability on NaN-filled scratch, masks of ones, exact zeros past each length.

The cases and their host-made inputs are tests/tacotron_cbhg_grad_cases.py (whose margin condition tests/test_tacotron_cbhg_grad_cpu.py
proves); every case's device passes and checker passes are computed once and shared."""
import functools

import numpy as np
import pytest

from helpers import assert_bar, first_mismatch, run_grad_handle, same_outputs
from tacotron_cbhg_grad_cases import CASES, CHAIN_CASES, MARGIN, host_case

pytestmark = pytest.mark.gpu

RTOL = 5e-5          # float32 kernel vs float64 restatement, per output, relative to its maximum (tests/test_tacotron_targets_gpu.py)


class _Case(object):
    """a host case with its model on the device and the two C entries on (row ranges of) its inputs"""

    def __init__(self, name):
        import torch
        from twvk_amd.tacotron import Tacotron
        self.h = host_case(name)
        self.torch = torch
        self.m = Tacotron(self.h.hp, num_speakers=self.h.speakers)
        self.m.load_weights(self.h.w)

    def _run(self, which, N, t, poison, call):
        def check_route(route):
            assert route["kernel"] == "cg_bigru" and route["side"] == ("post" if which else "encoder") and route["weights"] == "registers", route
        return run_grad_handle(self.m, "twv_tacotron_cbhg_grad", (which, N, t), check_route, poison, call)

    def encoder(self, d_memory=None, masks="case", rows=None, poison=False):
        from twvk_amd import _lib
        from twvk_amd.tacotron import _ptr, _stream, encoder_grad_layout
        h, m, torch, dev = self.h, self.m, self.torch, self.m.device
        sl = slice(0, h.N) if rows is None else rows
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[sl])).to(dev)
        mk = h.masks if isinstance(masks, str) else masks
        tok, ln, bh, init, dm = up(h.tok), up(h.ln), up(h.bh), up(h.init), up(h.d_memory if d_memory is None else d_memory)
        m1, m2 = (up(mk[0]), up(mk[1])) if mk is not None else (None, None)

        def call(g, ws, status, new):
            N = sl.stop - sl.start
            memory, grad = new(N, h.T, dm.shape[2]), new(m._blob.numel())
            d_bh, d_init = (new(N, bh.shape[1]), new(N, init.shape[1])) if bh is not None else (None, None)
            _lib.check(m._L.twv_tacotron_encoder_grad_run(g, _ptr(m._blob), _ptr(tok), _ptr(ln), _ptr(bh), _ptr(init), _ptr(m1), _ptr(m2), _ptr(dm),
                                                          _ptr(ws), _ptr(status), _stream(), _ptr(memory), _ptr(grad), _ptr(d_bh), _ptr(d_init)))
            out = {"memory": memory, "blob": grad}
            if bh is not None:
                out["d_before_highway"], out["d_rnn_init"] = d_bh, d_init
            return out
        out = self._run(0, sl.stop - sl.start, h.T, poison, call)
        return self._named(out, encoder_grad_layout(m.specs))

    def postnet(self, d_linear=None, rows=None, poison=False):
        from twvk_amd import _lib
        from twvk_amd.tacotron import _ptr, _stream, postnet_grad_layout
        h, m, torch, dev = self.h, self.m, self.torch, self.m.device
        sl = slice(0, h.N) if rows is None else rows
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a[sl])).to(dev)
        mel, dl = up(h.mel), up(h.d_linear if d_linear is None else d_linear)

        def call(g, ws, status, new):
            N = sl.stop - sl.start
            lin, grad, d_mel = new(N, h.TO, dl.shape[2]), new(m._blob.numel()), new(N, h.TO, mel.shape[2])
            _lib.check(m._L.twv_tacotron_postnet_grad_run(g, _ptr(m._blob), _ptr(mel), _ptr(dl), _ptr(ws), _ptr(status), _stream(), _ptr(lin),
                                                          _ptr(grad), _ptr(d_mel)))
            return {"linear": lin, "blob": grad, "d_mel": d_mel}
        out = self._run(1, sl.stop - sl.start, h.TO, poison, call)
        return self._named(out, postnet_grad_layout(m.specs))

    def _named(self, out, layout):
        """the tensors by name; a batch norm's (d_inv, d_shift) slot as (d_gamma, d_beta) through tacotron.bn_grad_from_inference_pair, the
        function Tacotron's methods use.  The checker side does not: tests/torch_tacotron_cbhg_grad_ref.py differentiates gamma and beta
        themselves, so the expected values are computed independently of that function."""
        from twvk_amd.tacotron import bn_grad_from_inference_pair
        inside = np.zeros(out["blob"].size, bool)
        for name, off, shp in layout:
            v = out["blob"][off:off + int(np.prod(shp))].reshape(shp)
            inside[off:off + v.size] = True
            if name.endswith("batch_normalization"):
                v = bn_grad_from_inference_pair(v, self.h.w[name])
            out[name] = v
        out["inside"] = inside
        return out

    @functools.lru_cache(maxsize=None)
    def encoder_hip(self):
        return self.encoder()

    @functools.lru_cache(maxsize=None)
    def postnet_hip(self):
        return self.postnet()

    @functools.lru_cache(maxsize=None)
    def forward(self):
        """the device's own teacher-forced pass of the case: (memory, mel, linear) as numpy"""
        h, m = self.h, self.m
        mel, lin, _ = m.forward_targets(h.tok, h.ln, h.spk, h.tgt, teacher_forced=True)
        memory = m.workspace_view(h.N, h.T, "memory").clone().view(h.N, h.T, -1)
        return memory.cpu().numpy(), mel.cpu().numpy(), lin.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(name):
    import torch
    assert torch.cuda.is_available()
    return _Case(name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_encoder_gradients_meet_the_bar(name):
    c = _case(name)
    h = c.h
    mem64, g64, rec = h.encoder_checker("float64")
    assert rec["relu_margin"] > MARGIN and rec["pool_gap"] > MARGIN, rec["relu_margin"]
    _, g32, _ = h.encoder_checker("float32")
    got = c.encoder_hip()
    assert_bar(name + " encoder", got, g64, g32)
    scale = float(np.abs(mem64).max())
    assert float(np.abs(got["memory"] - mem64).max()) <= RTOL * scale
    if h.forced and h.masks is None:
        assert float(np.abs(got["memory"].astype(np.float64) - c.forward()[0]).max()) <= RTOL * scale
    # slots outside the differentiated range read 0, the <PAD> row of the embedding too; outputs and deltas past a length are zeros
    assert not got["blob"][~got["inside"]].any() and got["blob"][got["inside"]].any()
    assert not got["embedding"][0].any() and got["embedding"][1:].any()
    for n, ln in enumerate(h.ln):
        assert not got["memory"][n, ln:].any() and got["memory"][n, :ln].any(), (name, n)


@pytest.mark.parametrize("name", sorted(CASES))
def test_postnet_gradients_meet_the_bar(name):
    c = _case(name)
    h = c.h
    lin64, g64, rec = h.postnet_checker("float64")
    assert rec["relu_margin"] > MARGIN and rec["pool_gap"] > MARGIN, rec["relu_margin"]
    _, g32, _ = h.postnet_checker("float32")
    got = c.postnet_hip()
    assert_bar(name + " post", got, g64, g32)
    scale = float(np.abs(lin64).max())
    assert float(np.abs(got["linear"] - lin64).max()) <= RTOL * scale
    if h.forced:
        assert float(np.abs(got["linear"].astype(np.float64) - c.forward()[2]).max()) <= RTOL * scale
    assert not got["blob"][~got["inside"]].any() and got["blob"][got["inside"]].any()


def test_linear_in_the_cotangent():
    c = _case("A-masked-tails")
    h = c.h
    for one, two, zero, fwd in ((c.encoder_hip(), c.encoder(d_memory=2.0 * h.d_memory), c.encoder(d_memory=np.zeros_like(h.d_memory)), "memory"),
                                (c.postnet_hip(), c.postnet(d_linear=2.0 * h.d_linear), c.postnet(d_linear=np.zeros_like(h.d_linear)), "linear")):
        for k in one:
            if k not in (fwd, "inside"):
                assert first_mismatch(2.0 * one[k], two[k]) is None, k
                assert not zero[k].any(), k
        assert first_mismatch(one[fwd], two[fwd]) is None


@pytest.mark.parametrize("name", ["A-masked-tails", "B-nine-utterances"])
def test_an_utterance_alone_gives_its_rows_of_the_batch(name):
    c = _case(name)
    enc, post = c.encoder_hip(), c.postnet_hip()
    for n in sorted({0, 1, c.h.N - 1}):
        alone = c.encoder(rows=slice(n, n + 1))
        for k in ("memory", "d_before_highway", "d_rnn_init"):
            assert first_mismatch(alone[k][0], enc[k][n]) is None, (name, n, k, first_mismatch(alone[k][0], enc[k][n]))
        alone = c.postnet(rows=slice(n, n + 1))
        for k in ("linear", "d_mel"):
            assert first_mismatch(alone[k][0], post[k][n]) is None, (name, n, k, first_mismatch(alone[k][0], post[k][n]))


def test_two_runs_give_the_same_bits_also_on_nan_filled_scratch():
    for name in ("A-masked-tails", "I-dropout-masks", "E-single-speaker"):
        c = _case(name)
        for first, run in ((c.encoder_hip(), c.encoder), (c.postnet_hip(), c.postnet)):
            same_outputs(first, run(), name + " second run")
            poisoned = run(poison=True)
            assert all(np.isfinite(v).all() for v in poisoned.values()), name
            same_outputs(first, poisoned, name + " NaN-filled workspace and outputs")


def test_masks_of_ones_are_no_masks():
    c = _case("A-masked-tails")
    ones = [np.ones((c.h.N, c.h.T, d), np.float32) for d in c.h.hp.enc_prenet_sizes]
    same_outputs(c.encoder_hip(), c.encoder(masks=ones), "masks of ones")


@pytest.mark.parametrize("name", ["A-masked-tails", "C-length-one", "B-nine-utterances"])
def test_a_cotangent_past_a_length_changes_nothing(name):
    c = _case(name)
    h = c.h
    d = h.d_memory.copy()
    rng = np.random.RandomState(3)
    for n, ln in enumerate(h.ln):
        d[n, ln:] = rng.randn(*d[n, ln:].shape).astype(np.float32)
    assert first_mismatch(d, h.d_memory) is not None
    same_outputs(c.encoder_hip(), c.encoder(d_memory=d), "cotangent past the lengths")


@pytest.mark.parametrize("prioritize", [False, True])
def test_linear_loss_cotangent(prioritize):
    import torch
    import torch_tacotron_cbhg_grad_ref as CG
    from twvk_amd import _lib
    from twvk_amd.tacotron import _ptr, _stream
    c = _case("A-masked-tails")
    h, m = c.h, c.m
    lin = c.forward()[2].astype(np.float32)
    tgt = h.lin_tgt.copy()
    tgt[0, 0, :7] = lin[0, 0, :7]                    # exact zeros of the difference: sign(0) = 0
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(m.device)
    out = torch.full(lin.shape, float("nan"), dtype=torch.float32, device=m.device)
    F, sr = h.hp.num_freq, float(h.hp.sample_rate)
    d_lin, d_tgt, d_co = up(lin), up(tgt), up(h.coeff)
    with torch.cuda.device(m.device):
        _lib.check(m._L.twv_tacotron_linear_loss_grad(_ptr(d_lin), _ptr(d_tgt), _ptr(d_co), h.N, h.TO, F, int(prioritize), sr, _ptr(out), _stream()))
        torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = CG.linear_loss_cotangent(lin, tgt, h.coeff, prioritize, sr, F)
    assert not got[0, 0, :7].any() and np.isfinite(got).all()
    # one float32 rounding of the factor, and of its product with loss_coeff
    assert float(np.abs(got - want).max()) <= 3 * 2.0 ** -24 * float(np.abs(want).max())
    lo, hi = int(165 / (sr * 0.5) * F), int(5000 / (sr * 0.5) * F)
    if prioritize:
        assert 0 < lo < hi < F and np.abs(got[1, 3, lo]) > 1.5 * np.abs(got[1, 3, lo - 1]) and np.abs(got[1, 3, hi - 1]) > 1.5 * np.abs(got[1, 3, hi])


@pytest.mark.parametrize("name", CHAIN_CASES)
def test_the_chain_from_the_loss_to_every_tensor(name):
    """forward_targets(teacher_forced=True) -> add_loss -> loss_gradients on the device, against the whole-model checker run from the tokens
    (the cases and why: tests/tacotron_cbhg_grad_cases.py CHAIN_CASES; their conditions are proved in tests/test_tacotron_cbhg_grad_cpu.py)"""
    import torch
    import torch_tacotron_cbhg_grad_ref as CG
    c = _case(name)
    h, m = c.h, c.m
    m.forward_targets(h.tok, h.ln, h.spk, h.tgt, teacher_forced=True)
    loss = m.add_loss(h.lin_tgt, h.coeff)["loss"]
    got = {k: v.cpu().numpy() for k, v in m.loss_gradients(h.lin_tgt, h.coeff).items()}
    assert m.cbhg_grad_route("encoder").startswith("kernel=cg_bigru side=encoder") and m.cbhg_grad_route("post").startswith("kernel=cg_bigru side=post")
    res = {torch.float64: h.chain_checker("float64"), torch.float32: h.chain_checker("float32")}
    l64, mel64, lin64, g64, rec = res[torch.float64]
    # the sign of every output - target difference must be beyond the reach of float32 rounding, the branches those of the float32 run
    assert rec["loss_margin"] > 1e-5 and rec["relu_margin"] > MARGIN and CG.same_branches(rec, res[torch.float32][4]), (rec["loss_margin"], rec["relu_margin"])
    assert rec["cumprod_margin"] > 1e-3, rec["cumprod_margin"]
    assert set(got) == set(g64), set(got) ^ set(g64)
    # every output is within RTOL of its maximum, and the loss a coeff-weighted mean of |output - target| of each side
    assert abs(loss - l64) <= RTOL * float(h.coeff.max()) * (float(np.abs(mel64).max()) + float(np.abs(lin64).max()))
    assert_bar(name + " chain", got, g64, res[torch.float32][3])
    m.forward_targets(h.tok, h.ln, h.spk, h.tgt, teacher_forced=False)
    for call in (lambda: m.loss_gradients(h.lin_tgt), lambda: m.encoder_grad(h.d_memory), lambda: m.postnet_grad(h.d_linear),
                 lambda: m.linear_loss_cotangent(h.lin_tgt)):
        with pytest.raises(ValueError):
            call()
