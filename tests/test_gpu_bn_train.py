"""GPU: the train-mode BatchNorm kernels ALONE (lt_bntrain.h: bn_partial_kernel, bn_finalize_kernel, bn_apply_kernel behind
bn_train_layer; the train-only first layers word_mlp1_kernel<false> / line_mlp1_kernel<false> and pos_encoder_bn around them),
through linetr_debug_bn_train, against float64 references written from the formula, at the channel widths, row strides and row
counts where their loops and chunks end.

Cases, input families, references and the bar -- max |gpu - ref64| <= 8 max(max |ref32 - ref64|, 2^-23 max |ref64|) per 64-row tile
of y and per statistics vector (batch mean, batch variance, running mean, running variance, alpha), a property of the CPU
references alone -- are in bn_cases.py, pinned to torch.nn.BatchNorm1d in double and to the oracle by test_bn_cases_cpu.py.
tools/bn_unit_report.py runs the same cases and writes the measured error / bar ratios to profiles/bn_unit_errors.txt.

What ran here for the first time: every width but 32, 64, 128, 256 and 512 (C = 96 / 100 / 252: threads of bn_partial_kernel
without a row; 256 < C < 512: a second channel pass for part of the block -- its barrier sat in a loop whose trip count differed
between the threads of a block, and for C = 260 between the lanes of a wave; the loop now runs to the block's bound with the loads
and stores guarded, same summation order), every row stride but ld = C (bn_train_layer now refuses a stride or a base that
bn_apply_kernel's 16-byte accesses cannot take), the chunking's edges and its empty trailing blocks.

The 'constant' family: a constant channel's variance q / n - mean^2 comes out as a rounding residue of either sign in float64; the
clamp makes it >= 0 and the test asks for 0 <= var inside the bar (all-zero channels: exactly 0), no NaN anywhere, y inside the bar.

What the file catches (each edit tried on a copy of the library, arithmetic only; "end to end" = test_train_mode_forward_golden
and test_train_mode_forward_vs_oracle_random_batches of tests/test_gpu_dropin.py, run against the same copy):
  unbiased variance in the normalisation      test_layer[*], test_layer_many_rows[*], test_encoder_chain[*]      end to end: caught too
  biased variance in the running update       test_layer[*], test_layer_many_rows[*], test_encoder_chain[*]      end to end: caught too
  the k < rp reduction skipped                test_layer[*], test_layer_many_rows[32-*], test_encoder_chain[*]   end to end: caught too
  momentum applied to the wrong term          test_layer[*], test_layer_many_rows[*], test_encoder_chain[*]      end to end: caught too
                                                                                     (not by its batch with momentum 0.5)
  the variance clamp removed                  test_layer[constant] (negative batch variance)                     end to end: NOT caught
  float accumulators in bn_partial_kernel     test_layer[*], test_layer_many_rows[*],                            end to end: NOT caught
                                              test_encoder_chain[line-widths1]
The end-to-end tests see the first four through the running statistics they compare to 2e-5; what they cannot see is anything that
only shows on inputs the network does not produce (a constant channel, |mean| / std in the hundreds) or at widths, strides and row
counts it does not run."""
import ctypes as C

import pytest
import torch

import bn_cases as BC
from attn_cases import MARKER, state_dict_t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

E_ARG, E_WORKSPACE = -1, -5

SMALL = [k for k in BC.layer_cases() if not BC.is_big(k)]
BIG = [k for k in BC.layer_cases() if BC.is_big(k)]
# every width once at a row count with five chunks of 67 rows, every wider stride, every family, one case with empty trailing blocks
TWICE = [k for k in SMALL if k[3] in (200, 333) and k[0] in ("workload", "sentinel", "constant")][::2] + [("sentinel", 260, 264, 32769, 0.1, 0.0)]


@pytest.fixture(scope="module")
def engines():
    from linetr_amd.engine import Engine
    made = {}

    def get(weights="calibrated", widths=BC.CHAIN_WIDTHS[0]):
        if (weights, widths) not in made:
            made[(weights, widths)] = Engine(BC.chain_state_dict(weights, widths)[0], "cuda:0", keyline_encoder=list(widths), bn_batch_stats=True)
        return made[(weights, widths)]
    return get


@pytest.fixture(scope="module")
def eng(engines):
    return engines()


# ---- one free-standing layer ----------------------------------------------------------------------------------------------------

def check_layer(eng, key):
    case = BC.layer_case(*key)
    got, nb = BC.launch_layer(eng, case)
    assert nb == min(512, max(1, case["rows"] // 64)), (key, nb)
    rows = BC.layer_errors(got, case)
    w = BC.worst(rows)
    print(f"bn_train {key}: nb {nb}, worst unit {w[0]} err {w[2]:.3e} bar {w[3]:.3e} ratio {w[2] / w[3] if w[3] else 0.0:.3f}")
    bad = [f"{key}: {m}" for m in BC.failures(rows)]
    if not all(bool(torch.isfinite(v).all()) for v in got.values()):
        bad.append(f"{key}: a result is not finite")
    if bool((got["var"] < 0).any()):
        bad.append(f"{key}: negative batch variance")
    if case["family"] == "constant" and bool((got["var"][torch.arange(case["C"]) % 4 == 2] != 0).any()):
        bad.append(f"{key}: an all-zero channel has a variance")
    if case["rows"] == 1 and (bool((got["var"] != 0).any()) or not torch.equal(got["mean"], case["z"][0])):
        bad.append(f"{key}: one row must give var = 0 and mean = the row")
    return bad


@pytest.mark.parametrize("family", BC.FAMILIES)
def test_layer(eng, family):
    """Every C in 4 .. 512 (widths that leave threads without a row or a channel, every rows-in-parallel class) at every row count
    around the chunking's edges 63 / 64 / 65, 127 / 128 / 129, 191 / 192 / 193 and at chunk sizes the rows in parallel do not
    divide (200, 333), ld = C, C + 4 and 2 C ('sentinel': +-1e4 between and behind the rows, bit-unchanged afterwards), momentum
    0, 0.1 and 1; the returned number of chunks is asserted for every case.  One row: var = 0, mean = the row, finite outputs."""
    bad = []
    for key in SMALL:
        if key[0] == family:
            bad += check_layer(eng, key)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("rows", BC.BIG_ROWS)
@pytest.mark.parametrize("C", BC.BIG_CHANNELS)
def test_layer_many_rows(eng, C, rows):
    """32 767 / 32 768 / 32 769 rows: 511 chunks, 512, and 512 of which the last seven own no row and must write zero partials;
    98 309 rows: chunks of 193 rows.  'workload' and 'offset' (|mean| / std = 256, 4096: what the float64 accumulators are for),
    and one case whose rows are 4 floats apart from the next."""
    bad = []
    keys = [key for key in BIG if key[1] == C and key[3] == rows]
    assert len(keys) == (2 if rows == 32769 else 1)
    for key in keys:
        bad += check_layer(eng, key)
    assert not bad, "\n".join(bad)


def test_same_case_twice_gives_the_same_bits(eng):
    """no atomics: y, the four statistics vectors, alpha and beta' are bit-identical from run to run"""
    for key in TWICE:
        case = BC.layer_case(*key)
        a, _ = BC.launch_layer(eng, case)
        b, _ = BC.launch_layer(eng, case)
        for k in a:
            assert torch.equal(a[k], b[k]), (key, k)


def test_without_the_batch_output_nothing_else_changes(eng):
    """batch = NULL: the same y, running statistics and alpha | beta' bit for bit, and the vector that was not handed over untouched"""
    for key in TWICE:
        case = BC.layer_case(*key)
        a, _ = BC.launch_layer(eng, case)
        b, nb = BC.launch_layer(eng, case, want_batch=False)
        assert nb == BC.n_chunks(case["rows"]) and b["mean"] is None
        for k in ("y", "run_mean", "run_var", "alpha", "beta2"):
            assert torch.equal(a[k], b[k]), (key, k)


# ---- the encoder chains ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("widths", BC.CHAIN_WIDTHS)
@pytest.mark.parametrize("enc", ["word", "line"])
def test_encoder_chain(engines, enc, widths):
    """pos_encoder_bn: the train-only first layer (pre-activations, no ReLU), three GEMMs without activation and four BatchNorm
    layers, against conv -> BatchNorm(batch) -> ReLU from the unfolded state dict; the output per 64-row tile, every layer's four
    statistics vectors each on their own."""
    bad = []
    for weights in BC.CHAIN_WEIGHTS:
        for rows in BC.CHAIN_ROWS:
            case = BC.chain_case(enc, weights, widths, rows)
            got, _, _, nb = BC.launch_chain(engines(weights, widths), case)
            assert nb == BC.n_chunks(rows)
            errs = BC.chain_errors(got, case)
            w = BC.worst(errs)
            print(f"bn chain {enc} w={weights} widths={widths} rows={rows}: worst unit {w[0]} err {w[2]:.3e} bar {w[3]:.3e} ratio {w[2] / w[3]:.3f}")
            bad += [f"{enc} w={weights} widths={widths} rows={rows}: {m}" for m in BC.failures(errs)]
    assert not bad, "\n".join(bad)


def test_chain_statistics_are_forward_trains(eng):
    """The same code on the same rows: the packed running and batch statistics of the two encoders' eight layers out of
    linetr_forward_train equal, bit for bit, what the two chains give on the same token and sub-line rows."""
    N, T, momentum = 37, 21, 0.1
    word, line = BC.chain_case("word", "calibrated", BC.CHAIN_WIDTHS[0], N * T), BC.chain_case("line", "calibrated", BC.CHAIN_WIDTHS[0], N)
    dev = eng.device
    g = BC._gen("forward_train", N, T)
    desc = torch.nn.functional.normalize(torch.randn((N, T, 256), generator=g), dim=2)
    n_enc = 2 * sum(BC.CHAIN_WIDTHS[0])
    running = torch.cat([word["running"], line["running"], torch.rand((eng.bn_stats_floats() - 2 * n_enc,), generator=g) + 0.5]).to(dev)
    pnt, score = word["inputs"]
    sub, resp, ang = line["inputs"]
    _, batch = eng.forward_train_tensors(sub.view(N, 2, 2).to(dev), pnt.view(N, T, 2).to(dev), resp.to(dev), ang.to(dev), desc.to(dev),
                                         score.view(N, T).to(dev), [0, 20, N], running, momentum, want_batch_stats=True)
    torch.cuda.synchronize()
    running, batch = running.cpu(), batch.cpu()
    for i, case in enumerate((word, line)):
        _, run, bat, _ = BC.launch_chain(eng, case)
        assert torch.equal(run, running[i * n_enc:(i + 1) * n_enc]), case["enc"]
        assert torch.equal(bat, batch[i * n_enc:(i + 1) * n_enc]), case["enc"]


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def _buffers(dev, rows=80, C_=32):
    mk = lambda *s: torch.full(s, MARKER, dtype=torch.float32, device=dev)
    return dict(z=mk(rows, 2 * C_), gamma=torch.ones(C_, device=dev), beta=torch.zeros(C_, device=dev), running=mk(2 * C_), batch=mk(2 * C_),
                affine=mk(2 * C_), pnt=torch.zeros((rows, 2), device=dev), score=torch.zeros(rows, device=dev),
                sub=torch.zeros((rows, 4), device=dev), resp=torch.zeros(rows, device=dev), ang=torch.zeros((rows, 2), device=dev),
                out=mk(rows, 256), run8=mk(960), bat8=mk(960), ws=torch.empty(8 << 20, dtype=torch.uint8, device=dev))


def raw(eng, b, which=-1, rows=64, C_=32, ld=32, momentum=0.1, ws_bytes=None, **over):
    a = dict(z=b["z"], gamma=b["gamma"], beta=b["beta"], in0=None, in1=None, in2=None, out=None, running=b["running"], batch=b["batch"],
             affine=b["affine"], ws=b["ws"])
    if which >= 0:
        a.update(z=None, gamma=None, beta=None, out=b["out"], running=b["run8"], batch=b["bat8"], affine=None,
                 in0=b["pnt"] if which == 0 else b["sub"], in1=b["score"] if which == 0 else b["resp"], in2=None if which == 0 else b["ang"])
    a.update(over)
    p = lambda t: t.data_ptr() if t is not None else None
    nb = C.c_int32(-1)
    code = eng._L.linetr_debug_bn_train(eng._h, which, p(a["z"]), rows, C_, ld, p(a["gamma"]), p(a["beta"]), p(a["in0"]), p(a["in1"]), p(a["in2"]),
                                        p(a["out"]), momentum, p(a["running"]), p(a["batch"]), p(a["affine"]), C.byref(nb), p(a["ws"]),
                                        a["ws"].numel() if ws_bytes is None and a["ws"] is not None else (ws_bytes or 0), None)
    return code, eng._L.linetr_last_error().decode()


def _untouched(b):
    torch.cuda.synchronize()
    return all(bool((b[k] == MARKER).all()) for k in ("z", "running", "batch", "affine", "out", "run8", "bat8"))


def test_refusals(eng):
    """What the entry point and bn_train_layer are not written for is refused with LINETR_E_ARG (a workspace that is too small:
    LINETR_E_WORKSPACE) and a message; nothing is launched (the outputs keep their marker)."""
    b = _buffers(eng.device)
    cases = [("C = 34", dict(C_=34, ld=36)), ("C = 516", dict(C_=516, ld=516)), ("C = 0", dict(C_=0, ld=4)), ("C = 2", dict(C_=2, ld=4)),
             ("ld < C", dict(ld=28)), ("ld = 34", dict(ld=34)), ("misaligned z", dict(z=b["z"].view(-1)[1:])), ("rows = -1", dict(rows=-1)),
             ("momentum -0.1", dict(momentum=-0.1)), ("momentum 1.5", dict(momentum=1.5)), ("momentum NaN", dict(momentum=float("nan"))),
             ("null z", dict(z=None)), ("null gamma", dict(gamma=None)), ("null beta", dict(beta=None)), ("null running", dict(running=None)),
             ("null workspace", dict(ws=None)), ("which = 2", dict(which=2)), ("which = -2", dict(which=-2)),
             ("word, null score", dict(which=0, in1=None)), ("line, null angle", dict(which=1, in2=None)), ("word, null output", dict(which=0, out=None)),
             ("line, misaligned output", dict(which=1, out=b["out"].view(-1)[1:])), ("word, null running", dict(which=0, running=None)),
             ("word, rows = -1", dict(which=0, rows=-1))]
    bad = []
    for what, kw in cases:
        code, text = raw(eng, b, **kw)
        if code != E_ARG or not text:
            bad.append((what, code, text))
    for which in (-1, 0, 1):
        need = eng._L.linetr_debug_bn_train_workspace_bytes(eng._h, which, 64)
        code, text = raw(eng, b, which=which, ws_bytes=need - 1)
        if code != E_WORKSPACE or not text:
            bad.append((f"which {which}: workspace one byte short", code, text))
    assert eng._L.linetr_debug_bn_train_workspace_bytes(eng._h, 2, 64) == -1 and eng._L.linetr_debug_bn_train_workspace_bytes(eng._h, -1, -1) == -1
    assert not bad, bad
    assert _untouched(b)
    code, text = raw(eng, b, rows=0)                        # no rows: fine, and nothing runs
    assert code == 0 and _untouched(b)
    code, text = raw(eng, b, ld=64)                         # the same buffers are served when nothing is wrong
    assert code == 0, text
    torch.cuda.synchronize()
    assert not bool((b["z"][:64, :32] == MARKER).any()) and bool((b["z"][:64, 32:] == MARKER).all()) and bool((b["z"][64:] == MARKER).all())


def test_inference_handle_is_refused():
    from linetr_amd.engine import Engine
    eng = Engine(state_dict_t("calibrated")[0], "cuda:0")
    b = _buffers(eng.device)
    for which in (-1, 0, 1):
        code, text = raw(eng, b, which=which)
        assert code == E_ARG and "inference" in text, (which, code, text)
    assert _untouched(b)
