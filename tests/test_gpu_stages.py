"""GPU: two stages from the middle of the forward pass ALONE (linetr_debug_stage, run by the forward pass's own host functions):
the descriptive layer's tail (value projection Watt, fc + LayerNorm, FFN with GELU, LayerNorm + line_pos) and the line-signature
network (0 .. 7 layers by every route of sig_network, final projection, L2 norm), against float64 references built from the
unfolded state dict -- so every weight linetr_create derives is checked with them.

Cases, references, teacher forcing and the bar -- max |gpu - ref64| <= 8 max(max |ref32 - ref64|, 2^-23 max |ref64|) per tensor
(tail) or per image and tensor (signature network), every step judged from the device's own input to it -- are in stage_cases.py;
tests/test_stage_cases_cpu.py pins the references to the oracle and shows that ten planted mistakes in the folds each break a bar.
tools/stage_unit_report.py runs the same cases and writes the measured error / bar ratios to profiles/stage_unit_errors.txt
(MI355X: bf16x6 at most 0.15 of a bar in the tail and 0.37 in the signature network; f32 at most 0.62 and 0.999, the latter on
line_desc of a 2-row image: 3.530e-7 against 3.534e-7)."""
import ctypes as C

import numpy as np
import pytest
import torch

import stage_cases as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

E_ARG = -1
DESC_TOL = 1e-4           # the project's stated tolerance on unit-norm descriptors (tests/test_gpu_parity.py, BASELINE.json north star)
_engines = {}


def engine(weights="calibrated", n_layers=7):
    from linetr_amd.engine import Engine
    key = (weights, n_layers)
    if key not in _engines:
        _engines[key] = Engine(S.weights_t(weights, n_layers)[0], "cuda:0", n_sig_layers=n_layers)
    return _engines[key]


class precision:
    def __init__(self, eng, mode):
        self.eng, self.mode = eng, mode

    def __enter__(self):
        self.eng.set_precision(self.mode)

    def __exit__(self, *exc):
        self.eng.set_precision("bf16x6")


def report(tag, rows):
    for w, u, n, e, b in rows:
        print(f"{tag} {w} [{u}] rows={n}: err {e:.3e} bar {b:.3e} ratio {e / b:.3f}")
    return [f"{tag}: {m}" for m in S.failures(rows)]


# ---- tail ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", S.TAIL_N)
@pytest.mark.parametrize("prec", ["f32", "bf16x6"])
@pytest.mark.parametrize("weights", S.WEIGHTS)
def test_tail(weights, prec, N):
    """att, o and zA of every family under their bars (o from the device's att, zA from the device's o); a second call gives the same
    bits; +-1e4 in the pad columns gives the bits of zeros there; the marker rows behind the outputs stay (launch_tail)."""
    eng, bad, got = engine(weights), [], {}
    with precision(eng, prec):
        for family in S.TAIL_FAMILIES:
            case = S.tail_case(family, N)
            got[family] = S.launch_tail(eng, case)
            again = S.launch_tail(eng, case)
            bad += [f"{family} {k}: two calls differ" for k in got[family] if not torch.equal(got[family][k], again[k])]
            bad += report(f"tail {weights} {prec} {family} N={N}", S.tail_errors(got[family], case, weights))
    bad += [f"pad {k}: not the bits of zeros in the pad columns" for k in got["pad"] if not torch.equal(got["pad"][k], got["normal"][k])]
    assert not bad, "\n".join(bad)


# ---- signature network --------------------------------------------------------------------------------------------------------

def run_sig(eng, case, weights, plan, tag, expect=None):
    L = int(eng.cfg["n_sig_layers"])
    desc, taps, used = S.launch_sig(eng, case, plan)
    desc2, taps2, _ = S.launch_sig(eng, case, plan)
    bad = [] if used == (plan if expect is None else expect) else [f"{tag}: plan {used} ran"]
    if not (torch.equal(desc, desc2) and torch.equal(taps, taps2)):
        bad.append(f"{tag}: two calls differ")
    return bad + report(f"{tag} {case['family']}", S.sig_errors(desc, taps, case, weights, L))


@pytest.mark.parametrize("prec,plan", [(p, k) for p in ("f32", "bf16x6") for k in S.FORCED[p]])
@pytest.mark.parametrize("n_layers", [7, 2])
@pytest.mark.parametrize("weights", S.WEIGHTS)
def test_sig_forced_plan(weights, n_layers, prec, plan):
    """Counts (0, 1, 2, 33, 129) by every route: every tap and line_desc under its bar, two runs bit-equal, sentinel rows and markers
    intact (launch_sig), and with the images of one parity filled with +-1e4 the other images stay under their bars."""
    eng, bad = engine(weights, n_layers), []
    with precision(eng, prec):
        for case in S.sig_cases():
            bad += run_sig(eng, case, weights, plan, f"sig {weights} L={n_layers} {prec} {S.PLAN_NAMES[plan]}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("prec", ["bf16x6", "f32"])
@pytest.mark.parametrize("counts,plan", S.DISPATCH)
def test_sig_dispatchers_choice(counts, plan, prec):
    """plan = -1: sig_attn_plan's own choice is reported and is the expected one; every tensor under its bar."""
    eng = engine()
    want = plan if prec == "bf16x6" else 0
    with precision(eng, prec):
        bad = run_sig(eng, S.sig_case("normal", counts), "calibrated", -1, f"sig dispatch {prec} {S.PLAN_NAMES[want]}", expect=want)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("prec", ["bf16x6", "f32"])
@pytest.mark.parametrize("n_layers", S.DEPTHS)
def test_sig_depth(n_layers, prec):
    """0 layers: the Wfin branch; 1 layer: Wfin2 without Wnext; 2 and 7: Wnext in between (the counts take small + fold_next)."""
    eng = engine("calibrated", n_layers)
    with precision(eng, prec):
        bad = run_sig(eng, S.sig_case("normal", S.SIG_COUNTS), "calibrated", -1, f"sig depth L={n_layers} {prec}",
                      expect=1 + S.FOLD_NEXT if prec == "bf16x6" else 0)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("prec", ["bf16x3", "f16x3"])
def test_sig_two_plane_modes(prec):
    """The two-plane modes promise the project's 1e-4 on unit-norm descriptors and nothing tighter: line_desc against the float64
    chain from z0, seven layers, the dispatcher's choice."""
    eng, case = engine(), S.sig_case("normal", S.SIG_COUNTS)
    with precision(eng, prec):
        desc, _, used = S.launch_sig(eng, case, -1)
    want = S.sig_chain(S._cast("calibrated", 7, torch.float64), case["z0"], case["cu"])[0]
    err = float((desc.double() - want).abs().max())
    print(f"sig {prec} plan {used}: max |line_desc - float64| = {err:.3e} (tolerance {DESC_TOL:g})")
    assert used == 1 + S.FOLD_NEXT and err < DESC_TOL


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def raw(eng, stage, N, in0, in1, cu, plan, outs, ws=None, ws_bytes=None, null_ws=False):
    cu = None if cu is None else np.ascontiguousarray(cu, dtype=np.int32)
    n_images = len(cu) - 1 if cu is not None else 1
    if ws is None and not null_ws:
        ws = eng._workspace("stage", eng._L.linetr_debug_stage_workspace_bytes(eng._h, N, n_images))
    if ws_bytes is None:
        ws_bytes = 1 << 40 if null_ws else ws.numel()
    used = C.c_int32(-7)
    p = lambda t: None if t is None else t.data_ptr()
    code = eng._L.linetr_debug_stage(eng._h, stage, N, p(in0), p(in1), None if cu is None else cu.ctypes.data, n_images, plan, p(outs[0]),
                                     p(outs[1]), p(outs[2]), C.byref(used), p(ws), ws_bytes, None)
    return code, eng._L.linetr_last_error().decode()


def test_refusals():
    """What the stage's buffers or kernels cannot serve, and every malformed call, is LINETR_E_ARG with a message; nothing is launched
    (the outputs keep their markers)."""
    eng = engine()
    dev = eng.device
    N = 961
    z = torch.zeros((N + 1, 256), device=dev)
    pooled, lpos = torch.zeros((N, 4, S.POOLW), device=dev), torch.zeros((N, 256), device=dev)
    outs = [torch.full((6 * N + 1, 256), S.MARKER, device=dev) for _ in range(3)]
    sig_outs = (outs[0], outs[1], None)
    one, big, two = S.cu_of([961]), S.cu_of([257, 3]), S.cu_of([40, 200])
    need = eng._L.linetr_debug_stage_workspace_bytes(eng._h, 240, 2)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    cases = [("fold_next above 960 rows", 1, 961, z, None, one, 1 + S.FOLD_NEXT, sig_outs),
             ("fold_next with split4", 1, 240, z, None, two, 2 + S.FOLD_NEXT, sig_outs),
             ("fold_next with fused", 1, 240, z, None, two, S.FUSED + S.FOLD_NEXT, sig_outs),
             ("fused, image above 256", 1, 260, z, None, big, S.FUSED, sig_outs),
             ("plan 5", 1, 240, z, None, two, 5, sig_outs), ("plan -2", 1, 240, z, None, two, -2, sig_outs),
             ("plan 16", 1, 240, z, None, two, 16, sig_outs), ("stage 2", 2, 240, z, None, two, -1, sig_outs),
             ("tail with a plan", 0, 240, pooled, lpos, None, 0, outs),
             ("cu_sub[0] != 0", 1, 240, z, None, np.array([1, 240]), -1, sig_outs),
             ("cu_sub not monotone", 1, 240, z, None, np.array([0, 300, 240]), -1, sig_outs),
             ("cu_sub does not end at N", 1, 241, z, None, two, -1, sig_outs),
             ("null z0", 1, 240, None, None, two, -1, sig_outs), ("null line_desc", 1, 240, z, None, two, -1, (None, outs[1], None)),
             ("null pooled", 0, 240, None, lpos, None, -1, outs), ("null lpos", 0, 240, pooled, None, None, -1, outs),
             ("misaligned z0", 1, 240, z[:, 1:], None, two, -1, sig_outs), ("misaligned line_desc", 1, 240, z, None, two, -1, (outs[0][:, 1:], None, None)),
             ("misaligned taps", 1, 240, z, None, two, -1, (outs[0], outs[1][:, 1:], None)),
             ("misaligned pooled", 0, 240, pooled[:, :, 1:], lpos, None, -1, outs), ("misaligned zA", 0, 240, pooled, lpos, None, -1, (None, None, outs[2][:, 1:]))]
    bad = []
    for what, stage, n, in0, in1, cu, plan, o in cases:
        code, text = raw(eng, stage, n, in0, in1, cu, plan, o)
        if code != E_ARG or not text:
            bad.append((what, code, text))
    for what, stage, in0, in1, cu, o in (("sig", 1, z, None, two, sig_outs), ("tail", 0, pooled, lpos, None, outs)):
        short = eng._L.linetr_debug_stage_workspace_bytes(eng._h, 240, 2 if stage else 1) - 1
        for name, args in (("one byte short", dict(ws=ws, ws_bytes=short)), ("misaligned", dict(ws=ws[8:], ws_bytes=need + 200)),
                           ("null", dict(null_ws=True))):
            code, text = raw(eng, stage, 240, in0, in1, cu, -1, o, **args)
            if code != E_ARG or not text:
                bad.append((f"{what}: workspace {name}", code, text))
    for prec, plans in (("f32", (1, 2, 3, S.FUSED, 1 + S.FOLD_NEXT)), ("bf16x3", (S.FUSED,)), ("f16x3", (S.FUSED,))):
        with precision(eng, prec):
            for plan in plans:
                code, text = raw(eng, 1, 240, z, None, two, plan, sig_outs)
                if code != E_ARG or not text:
                    bad.append((f"plan {plan} in {prec} mode", code, text))
    torch.cuda.synchronize()
    assert not bad, bad
    assert all(bool((o == S.MARKER).all()) for o in outs)


def test_training_mode_handle_is_refused():
    from linetr_amd.engine import Engine
    eng = Engine(S.weights_t("calibrated")[0], "cuda:0", bn_batch_stats=True)
    z = torch.zeros((8, 256), device=eng.device)
    out = torch.full((8, 256), S.MARKER, device=eng.device)
    for stage, in0, in1, cu in ((1, z, None, S.cu_of([8])), (0, torch.zeros((8, 4, S.POOLW), device=eng.device), z, None)):
        code, text = raw(eng, stage, 8, in0, in1, cu, -1, (out, None, None))
        assert code == E_ARG and text, (stage, code, text)
    torch.cuda.synchronize()
    assert bool((out == S.MARKER).all())
