"""The weight preparation (linetr_amd/csrc/lt_prepare.h) through linetr_debug_prepare, for tests/test_prepare_cpu.py and
tools/prepare_digest.py (which writes profiles/prepare_refactor_digest.txt).  Test infrastructure only; no device is touched.

One call of the accessor prepares once and returns the arena image, the pooling scalars behind it and the entry table; `prepared`
caches the result per configuration, so a test reads as many tensors as it likes for one preparation.

THE BAR of the fold tests.  Library and restatement both sum in float64 and round once to float32, in different orders (the library
term by term in ascending index order, the restatement by BLAS).  A length-256 float64 sum carries about 256 x 2^-53 relative error,
so the two roundings differ only where the sum sits that close to a float32 rounding boundary: probability about 256 x 2^-29 = 5e-7
per element.  Hence: every element within one float32 ulp (np.spacing) of the restatement, and at most 1e-5 of a tensor's elements --
one element of a tensor below 1e5 elements -- not bit-equal."""
import ctypes as C
import functools
import hashlib

import numpy as np

from linetr_amd import _native as nat
from linetr_amd.engine import DEFAULT_MODEL
import bn_cases as BC
import stage_cases as SC

E_WEIGHTS, E_CAPACITY = -3, -6             # LinetrStatus (include/linetr_hip.h)
GEMM, ST = 1, 2                            # LINETR_PREP_*
IMAGE_FLOATS = 12 << 20                    # the first guess of the image's size: a 7-layer arena is 10.0 M floats
CONFIGS = tuple((w, L, None, False) for w in SC.WEIGHTS for L in SC.DEPTHS) + (
    ("calibrated", 7, BC.CHAIN_WIDTHS[0], True), ("calibrated", 2, BC.CHAIN_WIDTHS[1], True))     # (weights, layers, widths, training mode)


def model_config(**model_cfg):
    cfg = {**DEFAULT_MODEL, **model_cfg}
    mc = nat.ModelConfig()
    mc.d_model, mc.n_heads, mc.d_inner = cfg["descriptor_dim"], cfg["n_heads"], cfg["d_inner"]
    mc.n_sig_layers, mc.n_desc_layers = cfg["n_sig_layers"], cfg["n_line_descriptive_layers"]
    for i, c in enumerate(cfg["keyline_encoder"]):
        mc.enc_channels[i] = c
    mc.norm_height, mc.norm_width = cfg["image_shape"]
    mc.bn_batch_stats = int(bool(cfg["bn_batch_stats"]))
    return mc


def call(sd, image, table, **model_cfg):
    """linetr_debug_prepare on a numpy state dict as Engine would hand it to linetr_create -> (status, floats, entries, message)"""
    L = nat.lib()
    names = [k.encode() for k in sd if not k.endswith("num_batches_tracked")]
    arrs = [np.ascontiguousarray(sd[k.decode()], dtype=np.float32) for k in names]
    n = len(names)
    n_floats, n_entries = C.c_int64(-1), C.c_int32(-1)
    code = L.linetr_debug_prepare(C.byref(model_config(**model_cfg)), n, (C.c_char_p * n)(*names), (C.c_void_p * n)(*[a.ctypes.data for a in arrs]),
                                  (C.c_int64 * n)(*[a.size for a in arrs]), nat.np_ptr(image) if image is not None else None,
                                  image.size if image is not None else 0, nat.np_ptr(table) if table is not None else None,
                                  table.size if table is not None else 0, C.byref(n_floats), C.byref(n_entries))
    return code, n_floats.value, n_entries.value, L.linetr_last_error().decode() if code else ""


class Prepared:
    """image: float32 [floats] (arena, then c_tok and s_cls); table: PREPARED_ENTRY_DTYPE records; self[name]: the tensor as [rows, cols]
    (a vector: [rows])"""

    def __init__(self, image, table):
        self.image, self.table = image, table
        self.entries = {r["name"].decode(): r for r in table}
        assert len(self.entries) == len(table), "an entry name appears twice"

    def __getitem__(self, name):
        r = self.entries[name]
        v = self.image[int(r["offset"]):int(r["offset"]) + int(r["rows"]) * int(r["cols"])]
        return v.reshape(int(r["rows"]), int(r["cols"])) if r["flags"] & GEMM or r["cols"] > 1 else v

    def arena_floats(self):
        return self.image.size - 8

    def digest(self):
        """one line per entry (name, offset, rows x cols, flags, SHA-256 of its floats) and one for the arena image as uploaded"""
        rows = [f"{n:8s} off {int(r['offset']):8d}  {int(r['rows']):5d} x {int(r['cols']):4d}  flags {int(r['flags'])}  "
                f"{hashlib.sha256(np.ascontiguousarray(self[n]).tobytes()).hexdigest()}" for n, r in self.entries.items()]
        return rows + [f"arena    {self.arena_floats()} floats  {hashlib.sha256(self.image[:self.arena_floats()].tobytes()).hexdigest()}"]


def prepare(sd, **model_cfg):
    image, table = np.empty(IMAGE_FLOATS, np.float32), np.zeros(512, nat.PREPARED_ENTRY_DTYPE)
    code, nf, ne, msg = call(sd, image, table, **model_cfg)
    if code == E_CAPACITY:
        image, table = np.empty(nf, np.float32), np.zeros(ne, nat.PREPARED_ENTRY_DTYPE)
        code, nf, ne, msg = call(sd, image, table, **model_cfg)
    if code:
        raise nat.NativeError(f"liblinetr_hip error {code}: {msg}")
    return Prepared(image[:nf].copy(), table[:ne].copy())


def config_state_dict(weights, n_layers, widths=None):
    """(numpy, torch) state dict of a configuration of CONFIGS"""
    if widths is None or tuple(widths) == BC.CHAIN_WIDTHS[0]:
        return SC.weights_t(weights, n_layers)
    sd, sd_t = BC.chain_state_dict(weights, tuple(widths))
    keep = lambda k: not k.startswith("selfattn.layers.") or int(k.split(".")[2]) < n_layers
    return {k: v for k, v in sd.items() if keep(k)}, {k: v for k, v in sd_t.items() if keep(k)}


def config_kwargs(n_layers, widths=None, training=False):
    return dict(n_sig_layers=n_layers, bn_batch_stats=training, **({"keyline_encoder": list(widths)} if widths else {}))


@functools.lru_cache(maxsize=None)
def prepared(weights, n_layers=7, widths=None, training=False):
    return prepare(config_state_dict(weights, n_layers, widths)[0], **config_kwargs(n_layers, widths, training))


def ulp_report(got, want):
    """(largest |got - want| in float32 ulps of `want`, elements that are not bit-equal, elements allowed to be) of two float32 arrays"""
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    return float(ulps.max(initial=0.0)), int((got.view(np.uint32) != want.view(np.uint32)).sum()), max(1, int(1e-5 * want.size))


def inside_bar(got, want):
    worst, differ, allowed = ulp_report(got, want)
    return worst <= 1.0 and differ <= allowed
