#!/usr/bin/env python3
"""Generate tests/golden/sig_attn_bwd.npz: the REAL reference's attention() (models/line_transformer.py:132-136) on seeded
query / key / value [2, 64, 4, 33] and the gradients torch autograd gives for a seeded upstream dO, in float32 and in float64.

Run in the build container only (needs the reference checkout, /root/reference or $LINETR_REFERENCE), on the CPU:

    python tests/golden/make_golden_sig_attn_bwd.py

The reference is imported as SURVEY.md Appendix D does (cv2 stub; the reference's packages first on the path).  Only data is written:
    q, k, v, dO [2, 64, 4, 33] float32 (the inputs of both runs); o, dq, dk, dv [2, 64, 4, 33] float64 of the float64 run on the same
    values; o_f32_err, dq_f32_err, dk_f32_err, dv_f32_err: max |float32 run - float64 run|, the float32 yardstick (the float32 arrays
    themselves would take the file past the size a committed file may have).

    python tests/golden/make_golden_sig_attn_bwd.py --double IN.npz OUT.npz

writes nothing to the fixture: it runs the reference's attention() in double on the fixture's q, k, v, dO and its MultiHeadedAttention in
double on the weights and inputs of IN.npz, and stores the results in OUT.npz, for tests/test_sig_attn_bwd_cpu.py (the reference's `models`
package cannot share a process with this repository's)."""
import os
import sys
import types

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("LINETR_REFERENCE", "/root/reference")
sys.path.insert(0, REFERENCE)   # FIRST on the path: `models` must be the reference's package

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models as _ref_models  # noqa: E402
assert _ref_models.__file__.startswith(REFERENCE.rstrip("/") + "/"), _ref_models.__file__
from models.line_transformer import MultiHeadedAttention, attention  # noqa: E402  (reference)

B, N_SUB, SEED = 2, 33, 9
KEYS = ("o", "dq", "dk", "dv")


def run(q, k, v, dO, dtype):
    qt, kt, vt = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (q, k, v))
    with torch.enable_grad():
        o, prob = attention(qt, kt, vt)
        o.backward(torch.tensor(dO, dtype=dtype))
    assert prob.shape == (q.shape[0], 4, q.shape[3], q.shape[3])
    return {"o": o.detach().numpy(), "dq": qt.grad.numpy(), "dk": kt.grad.numpy(), "dv": vt.grad.numpy()}


def run_mha(sd, query, source, g, shared):
    mod = MultiHeadedAttention(4, 256).double()
    mod.load_state_dict({key: torch.tensor(val, dtype=torch.float64) for key, val in sd.items()})
    qt = torch.tensor(query, dtype=torch.float64, requires_grad=True)
    st = qt if shared else torch.tensor(source, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        msg, _ = mod(qt, st, st)
        msg.backward(torch.tensor(g, dtype=torch.float64))
    out = {"message": msg.detach().numpy(), "d_query": qt.grad.numpy(), **{key: p.grad.numpy() for key, p in mod.named_parameters()}}
    if not shared:
        out["d_source"] = st.grad.numpy()
    return out


def double_check(inputs, path):
    """inputs: an .npz with mha<i>.<state_dict key>, mha<i>.query, mha<i>.source, mha<i>.g, mha<i>.shared for i = 0, 1"""
    f, cases = np.load(os.path.join(HERE, "sig_attn_bwd.npz")), np.load(inputs)
    out = {f"attn.{key}": val for key, val in run(f["q"], f["k"], f["v"], f["dO"], torch.float64).items()}
    names = sorted(MultiHeadedAttention(4, 256).state_dict())
    for i in (0, 1):
        sd = {key: cases[f"mha{i}.{key}"] for key in names}
        res = run_mha(sd, cases[f"mha{i}.query"], cases[f"mha{i}.source"], cases[f"mha{i}.g"], bool(cases[f"mha{i}.shared"]))
        out.update({f"mha{i}.{key}": val for key, val in res.items()})
    out["state_dict_keys"] = np.array(names)
    np.savez(path, **out)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--double":
        return double_check(sys.argv[2], sys.argv[3])
    rs = np.random.RandomState(SEED)
    q, k, v, dO = (rs.standard_normal((B, 64, 4, N_SUB)).astype(np.float32) for _ in range(4))
    f32, f64 = run(q, k, v, dO, torch.float32), run(q, k, v, dO, torch.float64)
    path = os.path.join(HERE, "sig_attn_bwd.npz")
    np.savez_compressed(path, q=q, k=k, v=v, dO=dO, **{key: f64[key] for key in KEYS},
                        **{f"{key}_f32_err": np.float64(np.abs(f32[key] - f64[key]).max()) for key in KEYS})
    for key in KEYS:
        print(f"{key}: max |.| {np.abs(f64[key]).max():.3e}, float32 error {np.abs(f32[key] - f64[key]).max():.2e}")
    print(f"{os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
