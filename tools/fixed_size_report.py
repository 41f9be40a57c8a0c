"""Measured error and time of the fixed-size training samples (csrc/lt_fixedsize.h through linetr_fixed_size /
Engine.fixed_size_batch) -- writes profiles/fixed_size_errors.txt and profiles/fixed_size_bench.txt:

    python tools/fixed_size_report.py [--out-dir profiles] [--iters 5]

Errors: every case of tests/golden/fixed_size.npz (the real conv_fixed_size), per key: exact keys as the number of differing elements,
desc_sublines as error / bar (tests/fixed_size_reference.py).
Time: B = 32 images of 480 x 640, max_sublines 250, max_tokens 21 (half of them padded, half truncated), the one native call against
the per-image path of tests/helpers.py::train_mode_batches -- preprocess per image, line_tokenizer per image for its pseudo lines,
torch.cat / a slice per key and image -- on the same GPU in the same process, alternating windows of `iters` calls between two
synchronisations; both sides start from detector rows and include the host pre-filter.  No time is fixed in advance."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fixed_size_reference as R  # noqa: E402
from sig_attn_bwd_report import compare  # noqa: E402
from workloads import synth  # noqa: E402

HW = (480, 640)
STREAM_TBS = 6.3          # the streaming rate profiles/adam_bench.txt quotes for this device, TB/s


def errors(eng):
    import test_gpu_fixed_size as T
    g = R.fixture()
    lines = []
    for name in R.cases(g):
        M = int(g[f"{name}_M"])
        out, _ = T.batch_call(eng, [g[f"{name}_lines"]], T.maps_of([g[f"{name}_seed"]]), M, pseudo_lines=[R.pseudo_of(g, name)])
        got = T.host(out)
        diff = {k: int((got[k] != g[f"{name}_{k}"]).sum()) for k in R.EXACT_KEYS}
        desc = got["desc_sublines"][0]
        step = int(g[f"{name}_desc_step"])
        err = float(np.abs(desc[::step] - g[f"{name}_desc_rows"]).max())
        err_sum = float(np.abs(desc.astype(np.float64).sum(-1) - g[f"{name}_desc_sum"]).max())
        lines.append(f"{name:14s} M {M:3d}  num_klns {int(got['num_klns'][0]):3d}  num_slns {int(got['num_slns'][0]):3d}   differing elements of the "
                     f"{len(diff)} exact keys: {sum(diff.values())}   desc_sublines {err:.3e} / {R.DESC_TOL:g} = {err / R.DESC_TOL:.3f}   "
                     f"channel sums {err_sum:.3e} / {R.DESC_SUM_TOL:g} = {err_sum / R.DESC_SUM_TOL:.3f}")
    return ("# every case of tests/golden/fixed_size.npz (the reference's conv_fixed_size on its own preprocess) through Engine.fixed_size_batch with the\n"
            "# fixture's pseudo lines: klines, length_klines, angles, the six exact per-sub-line keys and mat_klines2sublines must be array_equal;\n"
            "# desc_sublines as error / bar; written by tools/fixed_size_report.py on " + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines) + "\n")


def bench(eng, iters):
    from linetr_amd import line_process as lp
    from linetr_amd import util_lines as U
    B, M, T, TD = 32, 250, R.T, R.TD
    conf = {"min_length": 16, "max_sublines": -1, "token_distance": TD, "max_tokens": T, "remove_borders": 8}
    rows = [synth.synth_lines(1000 + b, 140 if b % 2 == 0 else 240, *HW, 17.0, 167.0 if b % 2 == 0 else 330.0) for b in range(B)]
    base = [synth.synth_dense_maps_np(1100 + i, *HW) for i in range(4)]
    dd = torch.from_numpy(np.concatenate([base[b % 4][0] for b in range(B)])).cuda()
    ds = torch.from_numpy(np.concatenate([base[b % 4][1] for b in range(B)])).cuda()
    keylines = [synth.array_to_keylines(r) for r in rows]
    pre = dict(remove_borders=8, min_length=16, max_keylines=-1, token_distance=TD, max_tokens=T)

    def native(pseudo=None):
        recs, cu_k, cu_n = eng.prefilter(rows, *HW, **pre)
        return eng.fixed_size_batch(recs, cu_k, cu_n, dd, ds, max_sublines=M, token_distance=TD, max_tokens=T, seed=1, pseudo_lines=pseudo), cu_n

    first, cu_n = native()
    pseudo = first["pseudo_lines"]
    ns = np.diff(cu_n)

    def per_image():
        outs = []
        for b in range(B):
            pred = {"dense_descriptor": dd[b:b + 1], "dense_score": ds[b:b + 1]}
            real = lp.preprocess(keylines[b], HW, pred, mask=None, conf=conf)
            one = {k: real[k][:, :M] for k in U.KEYS_PER_SUBLINE}
            if pseudo[b] is not None:
                tok = lp.line_tokenizer({k: v.copy() for k, v in pseudo[b].items()}, TD, T, pred, R.RESIZE)
                one = {k: torch.cat([one[k], tok[k]], dim=1) for k in U.KEYS_PER_SUBLINE}
            outs.append(one)
        return {k: torch.cat([o[k] for o in outs], dim=0) for k in U.KEYS_PER_SUBLINE}

    slow = per_image()
    same = all(torch.equal(slow[k], first[k]) for k in U.KEYS_PER_SUBLINE)
    (a, a0, a1), (t, t0, t1) = compare((lambda: native(pseudo), per_image), iters)
    # the native call alone, records already on the host: the device work and its launch
    recs, cu_k, cu_n = eng.prefilter(rows, *HW, **pre)
    recs = recs.copy()
    (c, c0, c1), = compare((lambda: eng.fixed_size_batch(recs, cu_k, cu_n, dd, ds, max_sublines=M, token_distance=TD, max_tokens=T, pseudo_lines=pseudo),), iters * 4)
    shapes = eng.fixed_size_shapes(B, M, T)
    written = 4.0 * sum(int(np.prod(sh)) for sh in shapes.values()) + 8.0 * B
    layout = 2.0 * dd.numel() * 4
    floor_ms = written / (STREAM_TBS * 1e12) * 1e3
    verdict = "the native call is faster" if a < t else "the native call is NOT faster than the per-image path"
    return (f"# B = {B} images of {HW[0]} x {HW[1]}, max_sublines {M}, max_tokens {T}: {int((ns < M).sum())} padded ({int(np.maximum(M - ns, 0).sum())} pseudo lines), "
            f"{int((ns >= M).sum())} truncated; NCHW descriptor maps; ms per call,\n# median of 5 alternating windows of {iters} calls each between two device synchronisations "
            f"(min .. max of the windows in brackets); same GPU, same process;\n# written by tools/fixed_size_report.py on {torch.cuda.get_device_name(0)}\n"
            f"pre-filter + Engine.fixed_size_batch (one native call)                      {a:9.3f} ms  [{a0:.3f} .. {a1:.3f}]\n"
            f"per image: preprocess + line_tokenizer(pseudo) + cat / slice, then cat      {t:9.3f} ms  [{t0:.3f} .. {t1:.3f}]   per-image / native {t / a:.2f}: {verdict}\n"
            f"the seven per-sub-line tensors of the two paths are bit-identical: {same}\n"
            f"Engine.fixed_size_batch alone (records on the host, pseudo lines given)    {c:9.3f} ms  [{c0:.3f} .. {c1:.3f}]\n"
            f"bytes the call must write: {written / 1e6:.1f} MB (desc_sublines {4.0 * np.prod(shapes['desc_sublines']) / 1e6:.1f} MB) = {floor_ms:.4f} ms at {STREAM_TBS} TB/s "
            f"-> the call alone is {c / floor_ms:.1f} x that; the NCHW layout pass in front moves another {layout / 1e6:.1f} MB\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    for name, make in (("fixed_size_errors.txt", lambda: errors(eng)), ("fixed_size_bench.txt", lambda: bench(eng, args.iters))):
        text = make()
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
