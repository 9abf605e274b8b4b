#!/usr/bin/env python
"""savfi_sepconv_bwd2_f32 against the float64 restatement on the cases of tests/test_sepconv2_gpu.py: max error over max|ref| per output,
next to the gate max(1e-5, 3 x the fp32 restatement's own error).  Writes profiles/sepconv_bwd2_parity.txt.  Needs a GPU."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import test_sepconv2_gpu as T          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'sepconv_bwd2_parity.txt'))
    out = ap.parse_args().out
    if not torch.cuda.is_available():
        raise RuntimeError("sepconv_bwd2_parity needs a GPU")
    lines = ["# python tools/sepconv_bwd2_parity.py   (%s; savfi_sepconv_bwd2_f32 vs tests/sepconv2_ref.sepconv_bwd2_f64; max err / max|ref|; "
             "gate = max(1e-5, 3 x the same figure of the restatement run in fp32))" % torch.cuda.get_device_name(0)]
    for case in T.CASES + [T.ABI_CASE]:
        res = T.measure(case)
        lines.append("B,C,Ho,Wo,K = %-20s " % (case,) + "   ".join("%s %.3e (gate %.3e, ratio %.3f)" % (n, e, g, e / g) for n, (e, g) in res.items()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
