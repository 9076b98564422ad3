#!/usr/bin/env python3
"""Records the answers of the four host-side convolution plan queries over the grid of tests/test_conv_plan_cpu.py:

    dycon_conv_gemm_workspace, dycon_conv_gemm_splits, dycon_conv_stats_chunks   one value per row of plan_grid(), in its order
    dycon_conv_wgrad_workspace                                                   one value per row of wgrad_grid() (the query takes
                                                                                 neither dtype nor scatter)

into conv_plans.json as four lists of integers.  The shapes are not stored: the grid functions are the key, and "rows" / "wgrad_rows"
hold their lengths.

The file pins what the library answered BEFORE the forward plan (conv_fwd_plan in csrc/conv.hip) replaced the separate ladders: run
it against a library built from that commit (3e2cd44), never against the tree it is meant to check.

    python tests/golden/make_golden_conv_plans.py /path/to/libdycon_hip.so
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from dycon_paper_replication_amd import _lib  # noqa: E402
from test_conv_plan_cpu import QUERIES, ask, plan_grid, wgrad_grid  # noqa: E402


def main(lib_path):
    lib = ctypes.CDLL(lib_path)
    for name in QUERIES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    fwd = [ask(lib, shape)[:3] for shape in plan_grid()]
    cols = {"workspace": [r[0] for r in fwd], "splits": [r[1] for r in fwd], "chunks": [r[2] for r in fwd],
            "wgrad_workspace": [ask(lib, shape)[3] for shape in wgrad_grid()]}
    out = os.path.join(HERE, "conv_plans.json")
    with open(out, "w") as f:      # one line per 14 x 14 block of (spatial, channels)
        f.write('{"rows": %d, "wgrad_rows": %d' % (len(fwd), len(cols["wgrad_workspace"])))
        for name, v in cols.items():
            lines = [",".join(map(str, v[i:i + 196])) for i in range(0, len(v), 196)]
            f.write(',\n"%s": [\n%s]' % (name, ",\n".join(lines)))
        f.write("}\n")
    print(f"{out}: {len(fwd)} rows, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
