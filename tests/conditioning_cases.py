"""The conditioning geometries the generation tests hold against the oracle: local-condition widths, upsampling lists and
global-condition widths away from hparams' (80, (5, 5, 12), 32).  Shared by tests/test_wavenet_conditioning_cpu.py (the inputs see
the channels and taps each row adds) and tests/test_wavenet_conditioning_gpu.py (every generation kernel, bit for bit).

Rows that vary L keep G = 32 and cardinality 2; rows that vary G keep L = 80 and (5, 5, 12).  NLC = ceil(L / 32) is the number of
32-channel chunks of a local-condition row, n_up the number of upsampling stages; the XCD kernels give each lc wave
min(4, (4 or 6) / NLC) layers, and the many-streams kernel is refused when (n_up + 1) * NLC > 12.

Common settings: dilations [1, 2, 4, 8, 16, 32, 64] cycled to the layer count (7 by default: the smallest at which every role of
the XCD kernels has work), the shifted head at weight scale 0.05, mel frames uniform(-4, 4), inputs from helpers.sensitive_mol /
sensitive_onehot.  T covers every phase of every upsampling stage twice, crosses two frame boundaries and ends inside a frame:
max(60, 2 * hop + 3) for the L rows; 603 for the G rows, whose last upsample0 tap is first read at row 240.  One mel frame more than
ceil(T / hop) is handed over."""
import zlib

import numpy as np

from helpers import make_case, make_model, mol_uniforms, sensitive_mol, sensitive_onehot
from sensitive_inputs import clamp_share

#        id        L    up              G   card   what it reaches
ROWS = {"l4": (4, (7,), 32, 2),           # one float4 of one chunk; n_up = 1; four layers per lc wave
        "l20": (20, (2, 3), 32, 2),       # partial first chunk; many frame boundaries inside a short call
        "l32f1": (32, (1, 5), 32, 2),     # exactly one chunk; a factor of 1 (its phase digit stays 0)
        "l36": (36, (2, 2, 3, 5), 32, 2),  # NLC = 2 with a 4-wide tail; n_up = 4; the many-streams kernel still fits (5 * 2)
        "l64": (64, (4, 4), 32, 2),       # two full chunks; two / three layers per lc wave
        "l68": (68, (5, 5, 12), 32, 2),   # smallest NLC = 3; the paired fast path with lanes 4 .. 31 of the second half dead
        "l96": (96, (5, 5, 12), 32, 2),   # full third chunk; the paired fast path at its Lc <= 96 edge
        "l100": (100, (3, 4), 32, 2),     # NLC = 4, tail of 4; the many-streams kernel fits (3 * 4 = 12) and takes the general body
        "l128": (128, (2, 3, 2, 2), 32, 2),  # the accepted maximum; (n_up + 1) * NLC = 20: the many-streams kernel is refused
        "g1": (80, (5, 5, 12), 1, 2),     # one global-condition channel
        "g5": (80, (5, 5, 12), 5, 2),     # not a multiple of 4
        "g33": (80, (5, 5, 12), 33, 2),   # second chunk of one channel
        "g64": (80, (5, 5, 12), 64, 2),   # both chunks full
        "g48emb": (80, (5, 5, 12), 48, 0)}  # the embedding passed as (B, 48) floats
L_ROWS = [r for r in ROWS if r.startswith("l")]
G_ROWS = [r for r in ROWS if r.startswith("g")]
HPARAMS = (80, (5, 5, 12), 32, 2)          # "l80": the default geometry, for the layer counts it has not run at

DIL7 = [1, 2, 4, 8, 16, 32, 64]
SHIFT, SCALE = 5.0, 0.05
DUMP_STEPS = 16


def geometry(rid):
    L, up, G, card = HPARAMS if rid == "l80" else ROWS[rid]
    return dict(L=L, up=up, G=G, gc_card=card)


def dilations(n_layers=7):
    return (DIL7 * ((n_layers + 6) // 7))[:n_layers]


def hop(rid):
    return int(np.prod(geometry(rid)["up"]))


def steps(rid):
    return max(60, 2 * hop(rid) + 3) if rid in L_ROWS else 603


def mel_frames(rid, T=None):
    h = hop(rid)
    return ((T or steps(rid)) + h - 1) // h + 1


class Case(object):
    """one model and its inputs: kw (for make_model), d, tensors, blob, mel, U (the oracle's upsampled rows, T of them), gc (ids, or
    the (B, G) embedding where the row has no table), first (the first input), u, want (the oracle's samples under u), and for a
    primed case `prime` (B, n), whose last column is `first`"""

    def figures(self):
        """(clamp share | None for class ids, share of the draws that carry an edge) of the oracle's output, for the parity table"""
        moved = (self.u != self.u0).reshape(self.B, self.T, -1).any(axis=2)
        return (clamp_share(self.want) if self.scalar else None), float(moved.mean())


_CASES = {}


def case(O, rid, B, n_layers=7, scalar=True, primed=False, builder=None, tag=""):
    """the case of row `rid` at B streams, built once per process and shared by the tests that ask for it (they leave it unchanged).
    builder(O, dilations, **kw) -> (d, tensors, blob) replaces helpers.make_case (the wide file's own, keyed by `tag`)."""
    key = (rid, B, n_layers, scalar, primed, tag)
    if key in _CASES:
        return _CASES[key]
    c = Case()
    c.rid, c.B, c.scalar, c.T = rid, B, scalar, steps(rid)
    c.dil = dilations(n_layers)
    c.kw = geometry(rid)
    if not scalar:
        c.kw.update(scalar_input=False, Q=256)
    if builder is None:
        c.d, c.tensors, c.blob = make_case(O, c.dil, scale=SCALE, shift=SHIFT, **c.kw)
    else:
        c.d, c.tensors, c.blob = builder(O, c.dil, **c.kw)
    L, G, card = c.kw["L"], c.kw["G"], c.kw["gc_card"]
    rng = np.random.RandomState(zlib.crc32(repr(key).encode()))
    c.mel = rng.uniform(-4, 4, (B, mel_frames(rid), L)).astype(np.float32)
    c.U = np.ascontiguousarray(O.upsample(c.d, c.blob, c.mel)[:, :c.T])
    c.gc = (np.arange(B) % 2).astype(np.int32) if card else (rng.randn(B, G) * SCALE).astype(np.float32)
    c.prime = None
    if primed:                                                       # generate.py:168-180: RF - 1 teacher-forced inputs, then the last one
        rf = O.receptive_field(c.d)
        c.prime = rng.uniform(-1, 1, (B, rf)).astype(np.float32) if scalar else rng.randint(256, size=(B, rf)).astype(np.int32)
        c.first = c.prime[:, -1].copy()
    else:
        c.first = (2 * rng.rand(B) - 1).astype(np.float32) if scalar else rng.randint(256, size=B).astype(np.int32)
    before = None if c.prime is None else c.prime[:, :-1]
    if scalar:
        c.u0 = mol_uniforms(B, c.T, c.d.O // 3)                      # what sensitive_mol starts from (its seed)
        c.u, c.want = sensitive_mol(O, c.d, c.blob, c.U, c.gc, c.first, B, c.T, prime=before)
    else:
        c.u0 = rng.random_sample((B, c.T))
        c.u, c.want = sensitive_onehot(O, c.d, c.blob, c.U, c.gc, c.first, c.u0, 1.0, prime=before)
    _CASES[key] = c
    return c


def model(c, B=None, **options):
    """the product model of a case (helpers.make_model) with the given kernel options (xcd, xcd_many, ...)"""
    return make_model(B or c.B, c.dil, c.tensors, **c.kw, **options)


# ---------------------------------------------------------------------------------------------------------------- single-channel mutants
def channel_mutants(c):
    """(label, tensors) with ONE slice of one conditioning tensor scaled by sensitive_inputs.MUTANT_FACTOR: the last input channel of
    lc_filter / lc_gate / gc_filter / gc_gate of layer 0 and of the last layer, the last tap of every upsampleN/kernel, the last row
    and the last column of gc_embedding (where the row has a table) -- the channels and taps the row's shape adds"""
    from sensitive_inputs import MUTANT_FACTOR

    def scaled(name, index):
        w = np.array(c.tensors[name], np.float32, copy=True)
        w[index] = w[index] * MUTANT_FACTOR
        t = dict(c.tensors); t[name] = w
        return t

    for layer in (0, c.d.n_layers - 1):
        for nm in ("lc_filter", "lc_gate", "gc_filter", "gc_gate"):
            name = "wavenet/dilated_stack/layer%d/dilation_layer/%s/kernel" % (layer, nm)
            yield "%s[last input channel]" % name, scaled(name, (slice(None), -1))
    for i in range(c.d.n_up):
        name = "wavenet/upsample%d/kernel" % i
        yield "%s[last tap]" % name, scaled(name, -1)
    if "wavenet/gc_embedding" in c.tensors:
        yield "wavenet/gc_embedding[last row]", scaled("wavenet/gc_embedding", -1)
        yield "wavenet/gc_embedding[last column]", scaled("wavenet/gc_embedding", (slice(None), -1))


def rerun(O, c, tensors):
    """the oracle's samples for other weights on the case's inputs (the upsampling kernels are weights too)"""
    blob = O.blob_from_tensors(c.d, tensors)
    U = O.upsample(c.d, blob, c.mel)[:, :c.T].copy()
    return O.generate_mol(c.d, blob, O.State(c.d, c.B), U, c.gc, c.first, c.u)
