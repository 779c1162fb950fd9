"""WaveNet scoring: the per-sample negative log-likelihood of given utterances, and a held-out loss.

Scoring is the reference's `add_loss` graph with reduce=False (wavenet/model.py:247-312, wavenet/mixture.py:27-81, train_mode=True):
'valid' convolutions, the local condition sliced from the front of every layer (model.py:79-80), targets audio[rf:].  An utterance of
T samples has T - rf values, nll[t] for t = rf .. T - 1.  It is not the incremental (generation) graph.

For a hop-aligned start s the graph on the crop (audio[s : s + n], mel[s / hop : (s + n) / hop]) gives exactly the whole utterance's
values at positions s + rf .. s + n - 1: the front slice of the local condition is shift-invariant at hop multiples.  So an utterance
is scored as hop-aligned windows with a halo of R = ceil(rf / hop) * hop samples (`plan`), packed into batches of `slots` windows for
twv_wavenet_score_windows; memory is bounded by (slots, window), never by the utterance.

    scorer = WaveNetScorer(net, window=None, slots=8)
    scorer.load_weights(tensors)                       # or a flat device blob: trainer.params / trainer.ema
    nll = scorer.score(audios, mels, gc_ids)           # list of 1-D float32 device tensors, each T_i - rf long
    loss, count = scorer.held_out_loss(audios, mels, gc_ids)

`plan` is host only (pure Python / numpy, no device)."""
import ctypes as C
from collections import namedtuple

import numpy as np

UTT, START, LENGTH, FIRST, LAST = 0, 1, 2, 3, 4

# table: int32 (n_batches, slots, 5) = {utterance index or -1 for an idle slot, first sample of the window, samples in the window,
# first kept position, last kept position (both inclusive, positions t of the utterance)}; n_windows: the windows in it
Plan = namedtuple("Plan", "table n_windows")


def halo(rf, hop):
    """R = ceil(rf / hop) * hop: the samples in front of a window's first kept position"""
    return -(-int(rf) // int(hop)) * int(hop)


def check_utterance(T, frames, rf, hop, what="utterance"):
    """the two host-side refusals: T <= rf (nothing to score) and T != frames * hop (assert_ready_for_upsampling,
    datasets/datafeeder_wavenet.py:38)"""
    if frames is not None and int(T) != int(frames) * int(hop):
        raise ValueError("%s: %d samples are not %d mel frames x hop size %d (datafeeder_wavenet.py:38)" % (what, T, frames, hop))
    if int(T) % int(hop):
        raise ValueError("%s: %d samples are not a multiple of the hop size %d" % (what, T, hop))
    if int(T) <= int(rf):
        raise ValueError("%s: %d samples do not exceed the receptive field %d: there is no position to score" % (what, T, rf))


def plan(lengths, window, rf, hop, slots):
    """The window table of a list of utterances (`lengths` in samples).  An utterance no longer than `window` is one window of its own
    length; a longer one is cut at a stride of window - R, its last window shifted back to end at T.  Window k keeps the positions the
    windows before it have not kept (a position covered twice is kept once, by the earlier window).  Windows go to the slots in order,
    `slots` per batch; the slots left over in the last batch are idle."""
    window, rf, hop, slots = int(window), int(rf), int(hop), int(slots)
    R = halo(rf, hop)
    if hop < 1 or slots < 1:
        raise ValueError("hop and slots must be >= 1")
    if window % hop:
        raise ValueError("window %d is not a multiple of the hop size %d" % (window, hop))
    if window <= rf:
        raise ValueError("window %d does not exceed the receptive field %d" % (window, rf))
    rows = []
    for i, T in enumerate(int(v) for v in lengths):
        check_utterance(T, None, rf, hop, "utterance %d" % i)
        if T <= window:
            rows.append((i, 0, T, rf, T - 1))
            continue
        if window <= R:
            raise ValueError("utterance %d (%d samples) needs more than one window: window %d must exceed the halo %d" % (i, T, window, R))
        start, last = 0, rf - 1
        while True:
            rows.append((i, start, window, last + 1, start + window - 1))
            last = start + window - 1
            if last == T - 1:
                break
            start = min(start + window - R, T - window)
    n = len(rows)
    table = np.zeros((-(-n // slots) if n else 0, slots, 5), np.int32)
    table[:, :, UTT] = -1
    for k, row in enumerate(rows):
        table[k // slots, k % slots] = row
    return Plan(table, n)


def default_window(rf, hop):
    """four halos: a quarter of every full window's rows are recomputed halo rows"""
    return 4 * halo(rf, hop)


class WaveNetScorer(object):
    def __init__(self, net, window=None, slots=8):
        import torch
        from . import _lib
        self.net = net
        self.rf, self.hop = int(net.receptive_field), int(net.hop_size)
        self.window = int(window) if window is not None else default_window(self.rf, self.hop)
        self.slots = int(slots)
        if self.slots < 1:
            raise ValueError("slots must be >= 1")
        if self.window % self.hop or self.window <= self.rf:
            raise ValueError("window %d must be a multiple of the hop size %d and exceed the receptive field %d" % (self.window, self.hop, self.rf))
        self.device = net.device
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.twv_wavenet_score_create(C.byref(net._dims), self.slots, self.window, C.byref(h)))
        self._h = h
        self.width = self._L.twv_wavenet_score_output_width(h)
        self.params = None
        self._ws = None
        self.frames = self.window // self.hop
        self.n_params = int(sum(int(np.prod(shape)) for _, shape in net.specs))
        self._torch = torch

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.twv_wavenet_score_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def route(self):
        """which kernel families score() runs (twv_wavenet_score_route) as a dict of strings: lc (fused | staged), head (skinny | gemm),
        loss (mol<10> | mol<0> | softmax), width (32 | 64 | 128), carve_floats"""
        return dict(kv.split("=", 1) for kv in self._L.twv_wavenet_score_route(self._h).decode().split())

    def view(self, name):
        """what the last run() left in the workspace (twv_wavenet_score_view), a 2-D slice of the workspace tensor: "zc" the stacked skip
        input (slots * width, n_layers * dilation_channels), "y" the raw network output (slots * width, out channels).  Rows a slot
        does not have hold whatever the workspace held."""
        from . import _lib
        if self._ws is None:
            raise RuntimeError("no workspace yet: run() first")
        off, rows, cols = C.c_longlong(), C.c_longlong(), C.c_longlong()
        _lib.check(self._L.twv_wavenet_score_view(self._h, name.encode(), C.byref(off), C.byref(rows), C.byref(cols)))
        return self._ws[off.value:off.value + rows.value * cols.value].view(rows.value, cols.value)

    def load_weights(self, tensors):
        """a dict of the variables by name (weights.tensor_specs), or a flat float32 blob in that order (WaveNetTrainer.params / .ema)"""
        from . import weights as W
        torch = self._torch
        if isinstance(tensors, dict):
            blob = torch.from_numpy(W.flatten(self.net.specs, tensors))
        else:
            blob = torch.as_tensor(tensors, dtype=torch.float32).reshape(-1)
        if int(blob.numel()) != self.n_params:
            raise ValueError("the model has %d parameters, got %d" % (self.n_params, int(blob.numel())))
        self.params = blob.to(self.device).contiguous().clone()

    # ---- host-side checks and staging ----
    def _host_inputs(self, audios, mels, gc_ids):
        torch = self._torch

        def host(x, dtype):
            return x.detach().cpu().numpy().astype(dtype, copy=False) if isinstance(x, torch.Tensor) else np.asarray(x, dtype)
        audios = [host(a, np.float32).reshape(-1) for a in audios]
        mels = [host(m, np.float32) for m in mels]
        if len(audios) != len(mels):
            raise ValueError("%d utterances but %d mels" % (len(audios), len(mels)))
        gcs = [0] * len(audios) if gc_ids is None else [int(g) for g in host(gc_ids, np.int64).reshape(-1)]
        if len(gcs) != len(audios):
            raise ValueError("%d utterances but %d gc ids" % (len(audios), len(gcs)))
        card = self.net.global_condition_cardinality or 1
        for i, (a, m) in enumerate(zip(audios, mels)):
            if m.ndim != 2 or m.shape[1] != self.net.local_condition_channels:
                raise ValueError("utterance %d: mel must be (frames, %d), got %s" % (i, self.net.local_condition_channels, m.shape))
            check_utterance(len(a), len(m), self.rf, self.hop, "utterance %d" % i)
            if not 0 <= gcs[i] < card:
                raise ValueError("utterance %d: gc id %d outside [0, %d)" % (i, gcs[i], card))
        return audios, mels, gcs

    def stage(self, rows, audios, mels, gcs):
        """host arrays of one window batch (`rows`: one (slots, 5) slice of the plan's table): audio (slots, window), mel
        (slots, window / hop, num_mels), gc ids (slots) and lengths (slots), zero where a slot has nothing"""
        a = np.zeros((self.slots, self.window), np.float32)
        m = np.zeros((self.slots, self.frames, self.net.local_condition_channels), np.float32)
        g = np.zeros(self.slots, np.int32)
        lens = np.zeros(self.slots, np.int32)
        for s, (u, start, n, _, _) in enumerate(rows):
            if u >= 0:
                a[s, :n] = audios[u][start:start + n]
                m[s, :n // self.hop] = mels[u][start // self.hop:(start + n) // self.hop]
                g[s], lens[s] = gcs[u], n
        return a, m, g, lens

    def run(self, a, m, g, lens, nll=None):
        """twv_wavenet_score_windows on one staged batch -> nll (slots, window - rf) device tensor (`nll`: a buffer to write into)"""
        from . import _lib
        from .wavenet import _ptr, _stream
        torch = self._torch
        if self.params is None:
            raise RuntimeError("no weights: call load_weights first")
        lens = np.ascontiguousarray(lens, np.int32)
        with torch.cuda.device(self.device):
            if self._ws is None:
                self._ws = torch.empty(self._L.twv_wavenet_score_workspace_bytes(self._h) // 4, dtype=torch.float32, device=self.device)
            da, dm, dg = torch.from_numpy(a).to(self.device), torch.from_numpy(m).to(self.device), torch.from_numpy(g).to(self.device)
            if nll is None:
                nll = torch.empty((self.slots, self.width), dtype=torch.float32, device=self.device)
            _lib.check(self._L.twv_wavenet_score_windows(self._h, _ptr(self.params), _ptr(da), _ptr(dm), _ptr(dg),
                                                        lens.ctypes.data_as(C.c_void_p), _ptr(self._ws), _ptr(nll), _stream()))
        return nll

    def _batches(self, audios, mels, gcs):
        """yields (table rows of the batch, nll (slots, width) device tensor of the batch)"""
        for rows in plan([len(a) for a in audios], self.window, self.rf, self.hop, self.slots).table:
            yield rows, self.run(*self.stage(rows, audios, mels, gcs))

    def score(self, audios, mels, gc_ids=None):
        """audios: list of (T_i,) float in [-1, 1]; mels: list of (T_i / hop, num_mels); gc_ids: one speaker id per utterance ->
        list of 1-D float32 device tensors, nll_i[t - rf] for t = rf .. T_i - 1.  ValueError (before the device is touched) when an
        utterance has T <= rf or T != frames * hop."""
        torch = self._torch
        audios, mels, gcs = self._host_inputs(audios, mels, gc_ids)
        out = [torch.empty(len(a) - self.rf, dtype=torch.float32, device=self.device) for a in audios]
        for rows, nll in self._batches(audios, mels, gcs):
            for s, (u, start, _, first, last) in enumerate(rows):
                if u >= 0:
                    out[u][first - self.rf:last + 1 - self.rf] = nll[s, first - start - self.rf:last + 1 - start - self.rf]
        return out

    def held_out_loss(self, audios, mels, gc_ids=None):
        """(mean nll over every scored position of the list, their count): model.py:290's mean over whole utterances.  The sum is
        carried in float64 on the device (twv_wavenet_score_reduce per window batch, the batches added in order)."""
        from . import _lib
        from .wavenet import _ptr, _stream
        torch = self._torch
        audios, mels, gcs = self._host_inputs(audios, mels, gc_ids)
        total = torch.zeros(2, dtype=torch.float64, device=self.device)
        part = torch.zeros(2, dtype=torch.float64, device=self.device)
        for rows, nll in self._batches(audios, mels, gcs):
            lo = np.asarray([max(f - st - self.rf, 0) if u >= 0 else 0 for u, st, _, f, _ in rows], np.int32)
            hi = np.asarray([l + 1 - st - self.rf if u >= 0 else 0 for u, st, _, _, l in rows], np.int32)
            with torch.cuda.device(self.device):
                _lib.check(self._L.twv_wavenet_score_reduce(_ptr(nll), lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), self.slots,
                                                           self.width, _ptr(part), _stream()))
            total += part
        s, n = (float(v) for v in total.cpu())
        return (s / n if n else float("nan")), int(n)
