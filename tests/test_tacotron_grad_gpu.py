"""-m gpu: the Tacotron decoder gradients (twv_tacotron_decoder_grad_run, Tacotron.decoder_grad / mel_loss_cotangent) against the float64
autograd checker tests/torch_tacotron_grad_ref.py, held to the project's gradient bar (tests/train_cases.py RATIO / FLOOR: per tensor at most
8 x the float32 autograd run's own distance from float64, floor 5e-6 of the tensor's maximum), and the exact properties of the pass:
linearity in d_mel, causality of the tape, masking, per-utterance independence, repeatability on NaN-filled scratch, masks of ones.

The cases and their host-made inputs are tests/tacotron_grad_cases.py (default decoder widths, small encoder / post banks); every case's
device pass and checker passes are computed once and shared."""
import functools

import numpy as np
import pytest

from helpers import assert_bar, first_mismatch, run_grad_handle, same_outputs
from tacotron_grad_cases import CASES, R_, HostCase

pytestmark = pytest.mark.gpu

RTOL = 5e-5          # float32 kernel vs float64 restatement, per output, relative to its maximum (tests/test_tacotron_targets_gpu.py)
TINY = float(np.finfo(np.float32).tiny)


class _Case(HostCase):
    """a host case with its model on the device, a teacher-forced pass (which leaves memory and the initial states in the workspace), and
    the C entry on copies of those"""

    def __init__(self, name):
        import torch
        from twvk_amd.tacotron import Tacotron
        HostCase.__init__(self, name)
        self.m = Tacotron(self.hp, num_speakers=2)
        self.m.load_weights(self.w)
        self.fwd_mel = self.m.forward_targets(self.tok, self.ln, self.spk, self.tgt, teacher_forced=True)[0].cpu().numpy()
        self.memory = self.m.workspace_view(self.N, self.T, "memory").clone().view(self.N, self.T, -1)
        self.init = self.m.workspace_view(self.N, self.T, "decoder_init").clone().view(self.N, -1)
        self.torch = torch

    def run(self, d_mel=None, masks="case", rows=None, tgt=None, poison=False):
        """twv_tacotron_decoder_grad_run on (a row range of) the case -> dict of numpy outputs: the decoder tensors by name, d_memory, d_init, mel"""
        from twvk_amd import _lib
        from twvk_amd.tacotron import _ptr, _stream, decoder_grad_layout
        torch, m, dev = self.torch, self.m, self.m.device
        sl = slice(0, self.N) if rows is None else rows
        N = sl.stop - sl.start
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[sl])).to(dev)
        dm = up(self.d_mel if d_mel is None else d_mel)
        tg = up(self.tgt if tgt is None else tgt)
        mk = self.masks if isinstance(masks, str) else masks
        m1, m2 = (up(mk[0]), up(mk[1])) if mk is not None else (None, None)
        ln = up(self.ln)
        memory, init = self.memory[sl].contiguous(), self.init[sl].contiguous()

        def check_route(route):
            assert route["kernel"] == "tg_bptt" and route["attention"] == self.at and route["layers"] == str(self.hp.dec_layer_num), route

        def call(g, ws, status, new):
            mel, grad = new(N, self.steps * R_, self.hp.num_mels), new(m._blob.numel())
            d_memory, d_init = new(N, self.T, memory.shape[2]), new(N, init.shape[1])
            _lib.check(m._L.twv_tacotron_decoder_grad_run(g, _ptr(m._blob), _ptr(memory), _ptr(init), _ptr(ln), _ptr(tg), _ptr(dm), _ptr(m1),
                                                          _ptr(m2), _ptr(ws), _ptr(status), _stream(), _ptr(mel), _ptr(grad), _ptr(d_memory),
                                                          _ptr(d_init)))
            return {"d_memory": d_memory, "d_init": d_init, "mel": mel, "blob": grad}
        out = run_grad_handle(m, "twv_tacotron_decoder_grad", (N, self.T, self.steps), check_route, poison, call)
        for name, off, shp in decoder_grad_layout(m.specs):
            out[name] = out["blob"][off:off + int(np.prod(shp))].reshape(shp)
        return out

    @functools.lru_cache(maxsize=None)
    def hip(self):
        return self.run()

    @functools.lru_cache(maxsize=None)
    def checker(self, dtype_name):
        import torch_tacotron_grad_ref as G
        return G.decoder_vjp(self.w, self.names, self.dims, self.memory.cpu().numpy(), self.init.cpu().numpy(), self.ln, self.at, self.tgt,
                             self.d_mel, self.masks, dtype=getattr(self.torch, dtype_name))


@functools.lru_cache(maxsize=None)
def _case(name):
    import torch
    assert torch.cuda.is_available()
    return _Case(name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradients_meet_the_bar_and_the_recorded_forward_is_the_forward(name):
    c = _case(name)
    mel64, g64, rec = c.checker("float64")
    # where a float32 run may take the other branch of a clamp the comparison means nothing: the case must stay clear of both edges
    assert rec["cumprod_margin"] > 1e-3 and rec["min_one_minus_p"] >= TINY, rec
    if name.startswith("B"):
        assert rec["clamp_engaged"], "case B is there for the 1e-10 clamp"
    _, g32, _ = c.checker("float32")
    got = c.hip()
    assert_bar(name, got, g64, g32)
    scale = float(np.abs(mel64).max())
    assert float(np.abs(got["mel"] - mel64).max()) <= RTOL * scale
    if c.masks is None:
        assert float(np.abs(got["mel"].astype(np.float64) - c.fwd_mel).max()) <= RTOL * scale
    # tensors outside the decoder read 0
    inside = np.zeros(got["blob"].size, bool)
    from twvk_amd.tacotron import decoder_grad_layout
    for _, off, shp in decoder_grad_layout(c.m.specs):
        inside[off:off + int(np.prod(shp))] = True
    assert not got["blob"][~inside].any() and got["blob"][inside].any()


def test_linear_in_the_cotangent():
    c = _case("A-masked-tails")
    one, two, zero = c.hip(), c.run(d_mel=2.0 * c.d_mel), c.run(d_mel=np.zeros_like(c.d_mel))
    for k in one:
        if k != "mel":
            assert first_mismatch(2.0 * one[k], two[k]) is None, k
            assert not zero[k].any(), k
    assert first_mismatch(one["mel"], two["mel"]) is None


def test_tape_is_causal():
    """d_mel non-zero on steps <= k only: the target rows that feed steps > k change no output"""
    c = _case("A-masked-tails")
    k = 3
    d_mel = c.d_mel.copy()
    d_mel[:, (k + 1) * R_:] = 0.0
    tgt = c.tgt.copy()
    tgt[:, (k + 1) * R_ - 1:] = np.random.RandomState(7).uniform(-4.0, 4.0, tgt[:, (k + 1) * R_ - 1:].shape).astype(np.float32)
    a, b = c.run(d_mel=d_mel), c.run(d_mel=d_mel, tgt=tgt)
    assert first_mismatch(a["mel"], b["mel"]) is not None, "the changed targets must reach the later steps"
    assert first_mismatch(a["mel"][:, :(k + 1) * R_], b["mel"][:, :(k + 1) * R_]) is None
    same_outputs(a, b, "causality", skip=("mel",))
    assert a["d_memory"].any() and a["d_init"].any()


@pytest.mark.parametrize("name", ["A-masked-tails", "E-length-one", "C-nine-utterances"])
def test_no_gradient_past_a_length(name):
    c = _case(name)
    d = c.hip()["d_memory"]
    for n, ln in enumerate(c.ln):
        assert not d[n, ln:].any() and d[n, :ln].any(), (name, n)


@pytest.mark.parametrize("name", ["A-masked-tails", "C-nine-utterances"])
def test_an_utterance_alone_gives_its_rows_of_the_batch(name):
    c = _case(name)
    full = c.hip()
    for n in sorted({0, 1, c.N - 1}):
        alone = c.run(rows=slice(n, n + 1))
        for k in ("d_memory", "d_init", "mel"):
            assert first_mismatch(alone[k][0], full[k][n]) is None, (name, n, k, first_mismatch(alone[k][0], full[k][n]))


def test_two_runs_give_the_same_bits_also_on_nan_filled_scratch():
    for name in ("A-masked-tails", "H-dropout-masks"):
        c = _case(name)
        first = c.hip()
        same_outputs(first, c.run(), name + " second run")
        poisoned = c.run(poison=True)
        assert all(np.isfinite(v).all() for v in poisoned.values()), name
        same_outputs(first, poisoned, name + " NaN-filled workspace and outputs")


def test_masks_of_ones_are_no_masks():
    c = _case("A-masked-tails")
    ones = [np.ones((c.N, c.steps, d), np.float32) for d in c.hp.dec_prenet_sizes]
    same_outputs(c.hip(), c.run(masks=ones), "masks of ones")


def test_end_to_end_from_tokens():
    """forward_targets(teacher_forced=True) -> mel_loss_cotangent -> decoder_grad on the device, against the checker run from the tokens
    (encoder under no_grad) with the same cotangent, under the same bar"""
    import torch
    import torch_tacotron_grad_ref as G
    c = _case("A-masked-tails")
    coeff = np.array([1.0, 0.5, 2.0], np.float32)
    mel = c.m.forward_targets(c.tok, c.ln, c.spk, c.tgt, teacher_forced=True)[0]
    cot = c.m.mel_loss_cotangent(coeff)
    mel_np, cot_np = mel.cpu().numpy(), cot.cpu().numpy()
    want = np.sign(mel_np - c.tgt).astype(np.float32) * (coeff[:, None, None] / np.float32(mel_np.size))
    assert cot_np.dtype == np.float32 and first_mismatch(cot_np, want.astype(np.float32)) is None
    got = {k: v.cpu().numpy() for k, v in c.m.decoder_grad(cot).items()}
    assert c.m.decoder_grad_route().startswith("kernel=tg_bptt attention=bah_mon_norm")
    assert set(got) == set(c.names) | {"d_memory", "d_init", "mel"}
    res = {}
    for dt in (torch.float64, torch.float32):
        memory, init = G.encoder_side(c.w, c.dims, c.tok, c.ln, c.spk, dtype=dt)
        res[dt] = G.decoder_vjp(c.w, c.names, c.dims, memory, init, c.ln, c.at, c.tgt, cot_np, dtype=dt)
    mel64, g64, rec = res[torch.float64]
    assert rec["cumprod_margin"] > 1e-3 and rec["min_one_minus_p"] >= TINY, rec
    assert_bar("end-to-end", got, g64, res[torch.float32][1])
    assert float(np.abs(got["mel"] - mel64).max()) <= RTOL * float(np.abs(mel64).max())
    # the methods need a teacher-forced pass
    c.m.forward_targets(c.tok, c.ln, c.spk, c.tgt, teacher_forced=False)
    with pytest.raises(ValueError):
        c.m.decoder_grad(cot)
    with pytest.raises(ValueError):
        c.m.mel_loss_cotangent()
