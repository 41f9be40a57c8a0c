"""CPU: the premises of tests/test_gpu_adam.py (tests/adam_cases.py) -- the float64 restatement against torch.optim.Adam in float64, the
order written in include/linetr_hip.h against the bar, the bar's teeth, the host arithmetic of the bias corrections, and the optimizer's
refusals that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_cases as AC


@pytest.mark.parametrize("family", AC.FAMILIES)
def test_restatement_equals_torch_in_float64(family):
    """a handful of float64 roundings in another order: within 64 x 2^-53 max |value| of torch.optim.Adam in float64"""
    worst = 0.0
    for step in AC.steps_of(family):
        case = AC.make_case(family, step)
        mine = AC.adam_f64(case["p"], case["g"], case["m"], case["v"], step, **case["hyper"])
        theirs = AC.torch_adam(case, torch.float64)
        for key in ("p", "m", "v"):
            assert theirs[key].dtype == np.float64
            top = np.abs(theirs[key]).max()
            err = np.abs(mine[key] - theirs[key]).max()
            worst = max(worst, err / (2.0 ** -53 * top) if top else (0.0 if err == 0 else np.inf))
            assert err <= 64 * 2.0 ** -53 * top, (family, step, key, err, top)
    print(f"adam {family}: float64 restatement against torch.optim.Adam(float64), worst error {worst:.2f} x 2^-53 max |value| (allowed 64)")


@pytest.mark.parametrize("family", AC.FAMILIES)
def test_written_order_stays_under_the_bar(family):
    """float32 NumPy in the header's order (fmaf through float64) on every case; torch's own foreach path gives the single-tensor bits"""
    worst = 0.0
    for step in AC.steps_of(family):
        case = AC.make_case(family, step)
        ref64, ref32 = AC.refs(family, step)
        rows = AC.ratios(AC.adam_f32(case["p"], case["g"], case["m"], case["v"], step, **case["hyper"]), case["p"], ref64, ref32)
        assert not AC.failures(rows), (family, step, AC.failures(rows))
        worst = max(worst, AC.worst(rows))
        each = AC.torch_adam(case, torch.float32, foreach=True)
        single = AC.torch_adam(case, torch.float32, foreach=False)
        assert all(each[k].tobytes() == single[k].tobytes() for k in ("p", "m", "v")), (family, step)
        assert AC.worst(AC.ratios(single, case["p"], ref64, ref32)) <= 1.0 / AC.FACTOR
    print(f"adam {family}: float32 restatement of the written order, worst error / bar {worst:.3f}")


def test_zero_results_are_met_exactly():
    case = AC.make_case("zeros", 10)
    ref64, ref32 = AC.refs("zeros", 10)
    assert not ref64["update"].any() and not ref64["m"].any() and not ref64["v"].any()
    rows = dict((k, (e, b)) for k, e, b in AC.ratios(AC.adam_f32(case["p"], case["g"], case["m"], case["v"], 10, **case["hyper"]), case["p"], ref64, ref32))
    assert rows["update"] == (0.0, 0.0) and rows["m"] == (0.0, 0.0) and rows["v"] == (0.0, 0.0)
    off ={"p": case["p"], "m": case["m"] + np.float32(1e-30), "v": case["v"]}
    assert AC.failures(AC.ratios(off, case["p"], ref64, ref32)), "a bar of 0 lets nothing through"


@pytest.mark.parametrize("defect", AC.DEFECTS)
def test_the_bar_has_teeth(defect):
    """the same comparison fed the float32 restatement with one planted defect fails at least one case"""
    caught, worst = [], 0.0
    for family, step in AC.all_cases():
        case = AC.make_case(family, step)
        ref64, ref32 = AC.refs(family, step)
        with np.errstate(all="ignore"):
            rows = AC.ratios(AC.adam_f32(case["p"], case["g"], case["m"], case["v"], step, defect=defect, **case["hyper"]), case["p"], ref64, ref32)
        if AC.failures(rows):
            caught.append((family, step))
            finite = [AC.ratio(e, b) for _, e, b in rows if np.isfinite(AC.ratio(e, b))]
            worst = max([worst] + finite)
    print(f"adam defect '{defect}': caught by {len(caught)} of {len(AC.all_cases())} cases, worst finite error / bar {worst:.3g}")
    assert caught, defect


def test_bias_corrections_equal_torchs_doubles():
    """(lr, betas, step) -> step_size, bc2_sqrt: the binding's one function against torch's own expressions, and against what a
    torch.optim.Adam step on one element implies"""
    from linetr_amd import _native as nat
    for lr in (1e-3, 3e-4, 0.0, 1.0):
        for betas in (AC.BETAS, (0.0, 0.0), (0.5, 0.9), (0.95, 0.9999)):
            for step in (1, 2, 3, 10, 1000, 1000000, 2.0 ** 24):
                bias_correction1 = 1 - betas[0] ** float(step)
                bias_correction2 = 1 - betas[1] ** float(step)
                assert nat.adam_bias_corrections(lr, betas[0], betas[1], step) == (lr / bias_correction1, bias_correction2 ** 0.5)
                assert nat.adam_bias_corrections(lr, betas[0], betas[1], step) == AC.corrections(lr, betas, step)
    # one element with m = v = 0 and eps = 0 moves by step_size (1 - beta1) g / (sqrt((1 - beta2) g^2) / bc2_sqrt): what torch takes
    for step in (1, 7, 1000):
        case = {"p": np.zeros(1), "g": np.array([0.5]), "m": np.zeros(1), "v": np.zeros(1), "step": step,
                "hyper": dict(lr=AC.LR, betas=AC.BETAS, eps=0.0, weight_decay=0.0, decoupled_weight_decay=False)}
        step_size, bc2_sqrt = nat.adam_bias_corrections(AC.LR, *AC.BETAS, step)
        want = -step_size * (0.1 * 0.5) / (np.sqrt(0.001 * 0.25) / bc2_sqrt)
        assert abs(AC.torch_adam(case, torch.float64)["p"][0] - want) <= 8 * 2.0 ** -53 * abs(want)


def test_structs_match_the_header():
    from linetr_amd import _native as nat
    assert nat.ADAM_TENSOR_DTYPE.itemsize == 48
    assert [nat.ADAM_TENSOR_DTYPE.fields[k][1] for k in ("p", "g", "m", "v", "n", "step_size", "bc2_sqrt")] == [0, 8, 16, 24, 32, 40, 44]
    assert C.sizeof(nat.AdamHyper) == 48 and nat.AdamHyper.decoupled.offset == 40
    for name in ("linetr_adam_workspace_bytes", "linetr_adam_step", "linetr_grad_norm_workspace_bytes", "linetr_grad_norm"):
        assert name in nat.ABI
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "linetr_hip.h")).read()
    assert "} LinetrAdamTensor;" in hdr and "} LinetrAdamHyper;" in hdr and "#define LINETR_ABI_VERSION 6" in hdr
    # the chunk and block sizes the GPU tests place their edges at
    src = open(os.path.join(root, "linetr_amd", "csrc", "lt_adam.h")).read()
    assert int(re.search(r"constexpr int AD_CHUNK = (\d+);", src).group(1)) == AC.CHUNK
    assert int(re.search(r"constexpr int AD_THREADS = (\d+);", src).group(1)) == AC.THREADS
    sizes = AC.ragged_sizes(AC.CHUNK, AC.THREADS)
    assert sorted(set(sizes)) == sizes and sizes[0] == 0 and sizes[-1] == 2 * AC.CHUNK + 5


def test_optimizer_refuses_without_a_device():
    """what linetr_amd.optim.Adam refuses before any native call: torch's unimplemented options, a tensor lr, parameters off the device"""
    from linetr_amd.optim import Adam
    cpu = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="HIP device"):
        Adam(cpu)
    with pytest.raises(ValueError, match="HIP device"):
        Adam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    for option in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=option):
            Adam(cpu, **{option: True})
    with pytest.raises(ValueError, match="tensor"):
        Adam(cpu, lr=torch.tensor(1e-3))
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0), dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            Adam(cpu, **bad)
    assert issubclass(Adam, torch.optim.Optimizer)
