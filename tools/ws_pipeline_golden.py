#!/usr/bin/env python3
"""Records the plain-form outputs that tests/test_gpu_conv_ws_pipeline.py pins bit for bit: for each case of its BITWISE list, the
sha256 of y and one checksum per pixel row, for bf16 and fp32 y -> tests/golden/ws_pipeline_<case>.npz.  Run it on the build whose
output is the contract (the commit BEFORE a change of conv3x3_ws_kernel's tap loop), on an MI355X:
    python3 tools/ws_pipeline_golden.py [output directory, default tests/golden]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import test_gpu_conv_ws_pipeline as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    os.makedirs(out, exist_ok=True)
    dev = torch.device('cuda:0')
    for name in T.BITWISE:
        rec = {}
        for key, y_bf16 in (('bf16', True), ('f32', False)):
            y, _, launched = T.run_plain(name, y_bf16, dev)
            assert launched[0][0] == T.WS3, launched
            sha, rows = T.digest(y)
            rec[f'sha_{key}'], rec[f'rows_{key}'] = np.array(sha), rows
            print(f'{name} {key}: {launched[0]} sha256 {sha[:16]}... {rows.size} rows')
        np.savez(os.path.join(out, f'ws_pipeline_{name}.npz'), **rec)


if __name__ == '__main__':
    main()
