"""Old against new libdmvs build on the 3-D convolutions: same bits, same speed.

    python tools/conv3d_ab.py bits OLD.so NEW.so [cpu|cuda:0]
        every parametrisation of the conv3d / deconv3d forward tests of tests/test_ops.py, each with tune 0, DMVS_TUNE3D_PIECES4 and
        DMVS_TUNE3D_NO_PAIR, on both libraries (cpu: two builds of tests/hipemu): one JSON line {"cases", "equal"}, exit 1 unless all equal
    python tools/conv3d_ab.py verdict --aa AA.jsonl ... --ab AB.jsonl ... [--ab4 AB_PIECES4.jsonl ...]
        the rows of several passes of `CONV_LIB=old CONV_LIB_B=... CONV_3D_ONLY=1 python tools/conv_bench.py` (--aa: old against a
        second copy of old, --ab: old against new, --ab4: the same with DMVS_CONV3D_V16=0).  Per row, new / old is the median over its
        passes; it passes the per-row bound if it is <= 1 + max over the A/A passes of that row's |ratio - 1|, and the global bound if
        it is <= 1 + max over all rows and A/A passes of |ratio - 1|.  The verdict is the per-row one (the tighter)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

TESTS = ["test_conv3d", "test_conv3d_xcd_grouped_tiles", "test_conv3d_streamed_tiles", "test_conv3d_16_byte_halo_pieces",
         "test_conv3d_paired_kernel_weights_in_registers", "test_conv3d_two_chunk_paired_kernel", "test_conv3d_stride2_matrix_core_form",
         "test_conv3d_volumes_smaller_than_a_tile", "test_conv3d_single_output_channel", "test_deconv3d_matrix_core_form"]


class Recording:
    """an Ops whose conv3d() ORs `force` into the tune word and keeps every output"""
    def __init__(self, ops, force):
        self.ops, self.force, self.outs, self.device = ops, force, [], ops.device

    def conv3d(self, pc, x, *, tune=None, **kw):
        out = self.ops.conv3d(pc, x, tune=(self.ops.tune["conv3d"] if tune is None else tune) | self.force, **kw)
        self.outs.append(out.cpu())
        return out


def bits(old, new, device="cpu"):
    import test_ops as T
    from diffmvs_amd import _lib
    from diffmvs_amd.ops import Ops
    libs = [Ops(_lib.Lib(os.path.abspath(p)), device) for p in (old, new)]
    cases = equal = 0
    for name in TESTS:
        fn = getattr(T, name)
        (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
        for params in mark.args[1]:
            for force in (0, _lib.TUNE3D_PIECES4, _lib.TUNE3D_NO_PAIR):
                outs = []
                for ops in libs:
                    rec = Recording(ops, force)
                    fn(rec, *params)
                    outs.append(rec.outs)
                same = len(outs[0]) == len(outs[1]) and all(torch.equal(a, b) for a, b in zip(*outs))
                cases, equal = cases + 1, equal + same
                if not same:
                    print("DIFFERS:", name, params, "tune", force, file=sys.stderr)
    print(json.dumps({"device": str(device), "cases": cases, "equal": equal}))
    return cases == equal


def verdict(argv):
    files = {"--aa": [], "--ab": [], "--ab4": []}
    for a in argv:
        if a in files:
            cur = files[a]
        else:
            cur.append([json.loads(line) for line in open(a) if line.startswith("{")])
    ratios = lambda passes: {r["layer"]: [q["ratio_b_over_a"] for p in passes for q in p if q["layer"] == r["layer"]] for r in passes[0]}
    aa = ratios(files["--aa"])
    row_bound = {k: round(1.0 + max(abs(x - 1.0) for x in v), 4) for k, v in aa.items()}
    global_bound = max(row_bound.values())
    out = {"rounds_per_pass": "5 alternating rounds of 10 launches per library, median per library", "aa_passes": len(files["--aa"]),
           "global_bound": global_bound, "old_vs_old_copy": [{"layer": k, "ratios": v, "row_bound": row_bound[k]} for k, v in aa.items()]}
    failing = []
    for key, name in (("--ab", "old_vs_new"), ("--ab4", "old_vs_new_pieces4")):
        if files[key]:
            us = {r["layer"]: (r["us"], r["us_b"]) for r in files[key][-1]}
            rows = [{"layer": k, "ratios": v, "median": sorted(v)[len(v) // 2], "row_bound": row_bound[k], "last_pass_us_old_new": us[k]}
                    for k, v in ratios(files[key]).items()]
            for r in rows:
                r["within_row_bound"], r["within_global_bound"] = r["median"] <= r["row_bound"], r["median"] <= global_bound
            failing += [name + ": " + r["layer"] for r in rows if not r["within_row_bound"]]
            out[name] = rows
    out["failing_row_bound"] = failing
    out["verdict"] = "pass" if not failing else "fail"
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if sys.argv[1] == "bits":
        sys.exit(0 if bits(*sys.argv[2:]) else 1)
    verdict(sys.argv[2:])
