"""The weight preparation's result as a listing: one SHA-256 per table entry (with its offset, shape and flags) and one for the
arena image, for both weight sets at 0, 1, 2 and 7 signature layers and for two training-mode configurations (no GPU needed).
    python tools/prepare_digest.py [--time N] [OUT]
Two builds prepare alike when their listings are equal line for line ($LINETR_LIB selects the build); profiles/prepare_refactor_digest.txt
records the listing.  --time N: instead, N wall times in seconds of one seven-layer preparation of the calibrated weights."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import prepare_cases as PC  # noqa: E402


def listing():
    out = []
    for weights, n_layers, widths, training in PC.CONFIGS:
        out.append(f"== weights {weights}, {n_layers} signature layers, keyline_encoder {list(widths or PC.DEFAULT_MODEL['keyline_encoder'])}, "
                   f"{'training mode' if training else 'inference'}")
        out += PC.prepared(weights, n_layers, widths, training).digest()
    return out


def times(n):
    sd = PC.config_state_dict("calibrated", 7)[0]
    out = []
    for _ in range(n):
        t = time.perf_counter()
        PC.prepare(sd, n_sig_layers=7)
        out.append(time.perf_counter() - t)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--time"]:
        print(" ".join(f"{t:.4f}" for t in times(int(args[1]))))
    else:
        text = "\n".join(listing()) + "\n"
        open(args[0], "w").write(text) if args else sys.stdout.write(text)
