"""-m gpu: the decoder gradients at the softmax attention types and loc_sen (twv_tacotron_decoder_grad_create_any: bah_norm, bah, luong,
luong_scaled, loc_sen) against the float64 autograd checker tests/torch_tacotron_grad_ref.py under the project's gradient bar
(helpers.assert_bar), and the exact properties tests/test_tacotron_grad_gpu.py holds the monotonic types to, restated for the new kinds:
linearity in d_mel, causality, zeros past a length, per-utterance independence, repeatability on NaN-filled scratch, masks of ones, a
reshaped handle.  The cases are tests/tacotron_attention_grad_cases.py; every case's device pass and checker passes are computed once."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import assert_bar, first_mismatch, run_grad_handle, same_outputs
from tacotron_attention_grad_cases import CASES, HostCase
from tacotron_grad_cases import R_

pytestmark = pytest.mark.gpu

RTOL = 5e-5          # the recorded forward against float64, relative to its maximum (tests/test_tacotron_grad_gpu.py)
PREFIX = "twv_tacotron_decoder_grad"
KINDS = ("bah_norm-tails", "bah-tails", "luong-tails", "luong_scaled-tails", "loc_sen-tails")


class _AnyDoor(object):
    """the model as helpers.run_grad_handle reads it, with <prefix>_create answered by twv_tacotron_decoder_grad_create_any"""

    class _Lib(object):
        def __init__(self, L):
            self._L = L

        def __getattr__(self, name):
            return getattr(self._L, PREFIX + "_create_any" if name == PREFIX + "_create" else name)

    def __init__(self, m):
        self._L, self._h, self.device = self._Lib(m._L), m._h, m.device


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

    def _call(self, d_mel, masks, rows, tgt, steps=None):
        """the arguments of one twv_tacotron_decoder_grad_run on (a row range, the first `steps` steps of) the case -> call(g, ws, status, new)"""
        from twvk_amd import _lib
        from twvk_amd.tacotron import _ptr, _stream
        torch, m, dev = self.torch, self.m, self.m.device
        sl = slice(0, self.N) if rows is None else rows
        N, steps = sl.stop - sl.start, self.steps if steps is None else steps
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[sl][:, :steps * (R_ if a.ndim == 3 and a.shape[1] == self.steps * R_ else 1)])).to(dev)
        dm, tg = up(self.d_mel if d_mel is None else d_mel), up(self.tgt if tgt is None else tgt)
        mk = self.masks if isinstance(masks, str) else masks
        m1, m2 = (up(mk[0]), up(mk[1])) if mk is not None else (None, None)
        ln = torch.from_numpy(np.ascontiguousarray(self.ln[sl])).to(dev)
        memory, init = self.memory[sl].contiguous(), self.init[sl].contiguous()

        def call(g, ws, status, new):
            mel, grad = new(N, steps * R_, self.hp.num_mels), new(m._blob.numel())
            d_memory, d_init = new(N, self.T, memory.shape[2]), new(N, init.shape[1])
            _lib.check(m._L.twv_tacotron_decoder_grad_run(g, _ptr(m._blob), _ptr(memory), _ptr(init), _ptr(ln), _ptr(tg), _ptr(dm), _ptr(m1),
                                                          _ptr(m2), _ptr(ws), _ptr(status), _stream(), _ptr(mel), _ptr(grad), _ptr(d_memory),
                                                          _ptr(d_init)))
            return {"d_memory": d_memory, "d_init": d_init, "mel": mel, "blob": grad}
        return N, steps, call

    def _named(self, out):
        from twvk_amd.tacotron import decoder_grad_layout
        for name, off, shp in decoder_grad_layout(self.m.specs):
            out[name] = out["blob"][off:off + int(np.prod(shp))].reshape(shp)
        return out

    def run(self, d_mel=None, masks="case", rows=None, tgt=None, poison=False):
        """one run on a handle of its own (twv_tacotron_decoder_grad_create_any) -> dict of numpy outputs: the decoder tensors by name,
        d_memory, d_init, mel"""
        N, steps, call = self._call(d_mel, masks, rows, tgt)

        def check_route(route):
            assert route["kernel"] == "tg_bptt" and route["attention"] == self.at and route["layers"] == str(self.hp.dec_layer_num), route
        return self._named(run_grad_handle(_AnyDoor(self.m), PREFIX, (N, self.T, steps), check_route, poison, call))

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


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_meet_the_bar_and_the_recorded_forward_is_the_forward(name):
    from twvk_amd.tacotron import decoder_grad_layout
    c = _case(name)
    mel64, g64, _ = c.checker("float64")
    _, g32, _ = c.checker("float32")
    got = c.hip()
    assert_bar(name, got, g64, g32)
    scale = float(np.abs(mel64).max())
    assert float(np.abs(got["mel"] - mel64).max()) <= RTOL * scale
    if c.masks is None:
        assert float(np.abs(got["mel"].astype(np.float64) - c.fwd_mel).max()) <= RTOL * scale
    # every decoder-side tensor has a gradient (the one-step case: but the first prenet kernel, which only sees the zero go frame);
    # tensors outside the decoder read 0
    inside = np.zeros(got["blob"].size, bool)
    for k, off, shp in decoder_grad_layout(c.m.specs):
        inside[off:off + int(np.prod(shp))] = True
        assert got[k].any() or (c.steps == 1 and k == "decoder/decoder_prenet/dense_1/kernel"), k
    assert not got["blob"][~inside].any()


@pytest.mark.parametrize("name", KINDS)
def test_linear_in_the_cotangent(name):
    c = _case(name)
    one, two, zero = c.hip(), c.run(d_mel=2.0 * c.d_mel), c.run(d_mel=np.zeros_like(c.d_mel))
    for k in one:
        if k != "mel":
            assert first_mismatch(2.0 * one[k], two[k]) is None, k
            assert not zero[k].any(), k
    assert first_mismatch(one["mel"], two["mel"]) is None


@pytest.mark.parametrize("name", ["bah_norm-tails", "loc_sen-tails"])
def test_tape_is_causal(name):
    """d_mel non-zero on steps <= k only: the target rows that feed steps > k change no output"""
    c = _case(name)
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


@pytest.mark.parametrize("name", KINDS + ("bah_norm-length-one", "luong-nine-utterances", "bah_norm-two-positions-a-thread"))
def test_no_gradient_past_a_length(name):
    c = _case(name)
    d = c.hip()["d_memory"]
    for n, ln in enumerate(c.ln):
        assert not d[n, ln:].any() and d[n, :ln].any(), (name, n)


@pytest.mark.parametrize("name", KINDS + ("luong-nine-utterances",))
def test_an_utterance_alone_gives_its_rows_of_the_batch(name):
    c = _case(name)
    full = c.hip()
    for n in sorted({0, 1, c.N - 1}):
        alone = c.run(rows=slice(n, n + 1))
        for k in ("d_memory", "d_init", "mel"):
            assert first_mismatch(alone[k][0], full[k][n]) is None, (name, n, k, first_mismatch(alone[k][0], full[k][n]))


@pytest.mark.parametrize("name", KINDS + ("bah_norm-dropout-masks",))
def test_two_runs_give_the_same_bits_also_on_nan_filled_scratch(name):
    c = _case(name)
    first = c.hip()
    same_outputs(first, c.run(), name + " second run")
    poisoned = c.run(poison=True)
    assert all(np.isfinite(v).all() for v in poisoned.values()), name
    same_outputs(first, poisoned, name + " NaN-filled workspace and outputs")


@pytest.mark.parametrize("name", ["bah-tails", "loc_sen-tails"])
def test_masks_of_ones_are_no_masks(name):
    c = _case(name)
    ones = [np.ones((c.N, c.steps, d), np.float32) for d in c.hp.dec_prenet_sizes]
    same_outputs(c.hip(), c.run(masks=ones), "masks of ones")


def test_an_utterance_of_one_position_gives_nothing_to_the_score_side():
    """alpha = 1 whatever the score, so de is exactly 0: alone, the utterance leaves every tensor the score reads with an exactly zero
    gradient (and its memory position still receives the context's)"""
    c = _case("bah_norm-length-one")
    assert c.ln[1] == 1
    alone = c.run(rows=slice(1, 2))
    for k in c.names:
        if k.startswith("decoder/bahdanau_attention/") or k == "memory_layer/kernel":
            assert not alone[k].any(), k
    assert alone["d_memory"][0, 0].any() and not alone["d_memory"][0, 1:].any() and alone["decoder/attention_wrapper/gru_cell/gates/kernel"].any()


@pytest.mark.parametrize("name", ["luong_scaled-tails", "loc_sen-tails"])
def test_a_reshaped_handle_is_a_new_one(name):
    """big -> small -> big on ONE handle and one NaN-filled workspace: each run gives the bits of a handle created at those sizes"""
    import torch
    from twvk_amd import _lib
    c = _case(name)
    L, dev = c.m._L, c.m.device
    small = dict(rows=slice(1, 3), steps=3)
    want = {"big": c.hip()}
    N, steps, call = c._call(None, "case", small["rows"], None, small["steps"])
    want["small"] = c._named(run_grad_handle(_AnyDoor(c.m), PREFIX, (N, c.T, steps), lambda route: None, False, call))
    g = C.c_void_p()
    _lib.check(L.twv_tacotron_decoder_grad_create_any(c.m._h, c.N, c.T, c.steps, C.byref(g)))
    try:
        ws = torch.full((L.twv_tacotron_decoder_grad_workspace_bytes(g) // 4,), float("nan"), dtype=torch.float32, device=dev)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
        for which in ("big", "small", "big"):
            n_, s_, call = c._call(None, "case", None, None) if which == "big" else c._call(None, "case", small["rows"], None, small["steps"])
            _lib.check(L.twv_tacotron_decoder_grad_reshape(g, n_, c.T, s_))
            assert L.twv_tacotron_decoder_grad_workspace_bytes(g) // 4 <= ws.numel()
            with torch.cuda.device(dev):
                out = call(g, ws, status, new)
                torch.cuda.synchronize()
            same_outputs(want[which], c._named({k: v.cpu().numpy() for k, v in out.items()}), name + " reshaped to " + which)
        # a handle from _create_any reshapes as _create_any validates: the existing size limits, in the existing words
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: .*1 <= t_in <= 1024"):
            _lib.check(L.twv_tacotron_decoder_grad_reshape(g, c.N, 1025, c.steps))
    finally:
        L.twv_tacotron_decoder_grad_destroy(g)
