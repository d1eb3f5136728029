"""The convolution's routing decision (conv2d_route, csrc/conv.hip), replayed on the CPU against tests/golden/conv_routes.npz.

The table was recorded from the library BEFORE the seven routing functions were folded into conv2d_route (generator:
tests/golden/gen_golden.py conv_routes), through the two entry points that answer without a device: dsd_op_conv2d_gn in
query mode and dsd_conv_plan.  Nothing is dereferenced there, so the pointers are made-up aligned addresses.

Every row must come out as recorded: refusal (with its text), split-K factor, statistics chunks, structure, tile width,
scratch bytes — and the kernel name, with one rule.  The old code named a launch after the plan that MAY split, whether or
not the caller gave scratch; the route names what launches.  So a no_scratch row is held to the name the old code gave the
launch that may not re-plan (column `unsplit`: the same query recorded with DSD_NO_SPLITK=1, which made the old planner
return what it returned for a caller without scratch), and every other row to the name recorded for itself.
"""
import ctypes as C
import json
import os

import numpy as np

from diffusion_models_dsdiff_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.npz")

# columns of the inputs of one dsd_op_conv2d_gn query; gn: 0 none, 1 output statistics wanted, 2 input coefficients given
OP_IN = ("N", "H", "W", "Cin", "Cout", "ks", "stride", "ups", "bits", "pad_lo", "pad_total", "out_nchw", "emb_stride",
         "no_scratch", "gn")
PLAN_IN = ("N", "H", "W", "Cin", "Cout", "ks", "stride", "bits")
X, WGT, Y, EMB, SCALE, SHIFT, STATS = (0x10000 * i for i in range(1, 8))   # never dereferenced: query mode touches no device


def query_op(row):
    """-> (refusal text with the kernel name taken out, or "" when accepted; kernel name; split-K factor; statistics chunks)"""
    r = dict(zip(OP_IN, (int(v) for v in row)))
    ex = _lib.DsdConvEx(x_batch_stride=-1, pad_lo=r["pad_lo"], pad_total=r["pad_total"], y_ld=0, out_nchw=r["out_nchw"],
                        emb_stride=r["emb_stride"], no_scratch=r["no_scratch"], ksplit=0)
    gn = _lib.DsdConvGn(gn_scale=SCALE if r["gn"] == 2 else None, gn_shift=SHIFT if r["gn"] == 2 else None,
                        stats=STATS if r["gn"] == 1 else None, stats_doubles=1 << 60 if r["gn"] == 1 else 0, stats_chunks=0, query=1)
    L = _lib.lib()
    rc = L.dsd_op_conv2d_gn(X, r["N"], r["H"], r["W"], r["Cin"], WGT, None, r["Cout"], r["ks"], r["stride"], r["ups"], EMB, None,
                            r["bits"], C.byref(ex), C.byref(gn), Y, None)
    name = ex.kernel.decode()
    text = L.dsd_last_error().decode() if rc else ""
    return (text.replace(name, "{kernel}") if name else text), name, ex.ksplit, gn.stats_chunks


def query_plan(row):
    st, nt, ks, sb = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
    _lib.check(_lib.lib().dsd_conv_plan(*(int(v) for v in row), C.byref(st), C.byref(nt), C.byref(ks), C.byref(sb)))
    return st.value, nt.value, ks.value, sb.value


def test_every_recorded_route_is_reproduced():
    assert "DSD_NO_SPLITK" not in os.environ and "DSD_FORCE_NT" not in os.environ   # (they change the plan for the whole process)
    g = np.load(GOLDEN)
    names, texts = json.loads(str(g["names"])), json.loads(str(g["texts"]))
    op_in, op_out = g["op_in"], g["op_out"]     # op_out: text, name, ksplit, stats_chunks, unsplit (indices into texts / names)
    assert len(op_in) == len(op_out) > 100000 and op_in.shape[1] == len(OP_IN)
    ns = OP_IN.index("no_scratch")
    bad, renamed = [], 0
    for row, (t, n, ks, sc, un) in zip(op_in, op_out):
        text, name, ksplit, chunks = query_op(row)
        want = names[un] if row[ns] else names[n]       # the rule of the module docstring, and the only one
        renamed += want != names[n]
        if (text, name, ksplit, chunks) != (texts[t], want, ks, sc):
            bad.append((dict(zip(OP_IN, row.tolist())), (text, name, ksplit, chunks), (texts[t], want, int(ks), int(sc))))
    assert not bad, f"{len(bad)} of {len(op_in)} rows differ, the first: {bad[:3]}"
    assert renamed == int(g["renamed"])     # (how many rows the rule touches is part of the record)
    plan_in, plan_out = g["plan_in"], g["plan_out"]
    assert len(plan_in) == len(plan_out) > 5000
    bad = [(r.tolist(), query_plan(r), tuple(o.tolist())) for r, o in zip(plan_in, plan_out) if query_plan(r) != tuple(o.tolist())]
    assert not bad, f"{len(bad)} of {len(plan_in)} plans differ, the first: {bad[:3]}"
