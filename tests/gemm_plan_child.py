"""Descriptor builder of tests/test_cpu_gemm_plan.py, and its child process: the library reads its environment knobs once per process, so
every knob setting plans the ten bf16-output GEMMs of one base transformer layer (the cases of tools/step_gemm_tiles.py) in a process of
its own and prints the plans as one JSON line.  Host only: the descriptors carry dummy 16-byte-aligned addresses that nothing dereferences."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from aptai_amd import _lib, ops  # noqa: E402

BIAS, GELU, RESIDUAL, DROPOUT, DGELU, PRE_DGELU, MUL_AUX, RESIDUAL_F32 = (ops.EPI_BIAS, ops.EPI_GELU, ops.EPI_RESIDUAL, ops.EPI_DROPOUT,
                                                                          ops.EPI_DGELU, ops.EPI_PRE_DGELU, ops.EPI_MUL_AUX, ops.EPI_RESIDUAL_F32)
LAYOUTS = {"NT": (0, 0), "NN": (0, 1), "TN": (1, 1), "TT": (1, 0)}     # (a_kmajor, b_kmajor): Linear forward, dgrad, wgrad, not built


def make_desc(M, N, K, layout="NT", out="bf16", flags=0, *, split_k=1, accumulate=False, batch=None, tile=0, out_pre=False, colscale_n=0,
              sk=False, workspace=True):
    """One aptai_gemm_desc with dense leading dimensions and every pointer its flags need."""
    d = ops.GemmDesc()
    d.a_kmajor, d.b_kmajor = LAYOUTS[layout]
    d.out_f32 = int(out == "f32")
    d.M, d.N, d.K = M, N, K
    d.A, d.lda = 0x10000, (M if d.a_kmajor else K)
    d.B, d.ldb = 0x20000, (N if d.b_kmajor else K)
    d.C, d.ldc = 0x30000, N
    d.flags = flags
    if flags & BIAS:
        d.bias = 0x40000
    if flags & (RESIDUAL | RESIDUAL_F32):
        d.residual, d.ldr = 0x50000, N
    if flags & (DGELU | MUL_AUX):
        d.aux, d.ldaux = 0x60000, N
    if out_pre:
        d.out_pre = 0x70000
    if flags & DROPOUT:
        d.dropout_p, d.seed = 0.1, 1
    d.split_k, d.accumulate, d.tile, d.colscale_n, d.colscale = split_k, int(accumulate), tile, colscale_n, 0.125
    if batch is not None:
        d.batch_outer, d.batch_inner = batch
    if d.out_f32 and (split_k > 1 or accumulate) and workspace:
        d.workspace, d.workspace_bytes = 0x80000, _lib.lib().aptai_gemm_workspace_bytes(M, N, split_k)
    if sk:
        d.sk_workspace, d.sk_workspace_bytes = 0x90000, _lib.lib().aptai_gemm_sk_workspace_bytes()
    return d


def plan(d):
    """(tile, nbatch, nsplit, ktiles_per_split, raster_gm, split column) of aptai_gemm_plan."""
    p = ops.gemm_plan(d)
    return (p.tile, p.nbatch, p.nsplit, p.ktiles_per_split, p.raster_gm, p.split_n)


M_, H_, I_ = 8192, 768, 3072
BASE_LAYER = [                                                                                       # tools/step_gemm_tiles.py, in its order
    (M_, 3 * H_, H_, "NT", "bf16", BIAS, dict(colscale_n=H_)),                                       # fwd qkv
    (M_, H_, H_, "NT", "bf16", BIAS | RESIDUAL | DROPOUT, {}),                                       # fwd out
    (M_, I_, H_, "NT", "bf16", BIAS | GELU | DROPOUT | PRE_DGELU, dict(out_pre=True)),               # fwd ffn1
    (M_, H_, I_, "NT", "bf16", BIAS | RESIDUAL | DROPOUT, {}),                                       # fwd ffn2
    (M_, I_, H_, "NN", "bf16", MUL_AUX, {}),                                                         # bwd ffn2
    (M_, H_, I_, "NN", "bf16", RESIDUAL, {}),                                                        # bwd ffn1, joining the residual gradient
    (M_, H_, I_, "NN", "bf16", 0, {}),                                                               # bwd ffn1
    (M_, H_, H_, "NN", "bf16", 0, {}),                                                               # bwd out
    (M_, H_, 3 * H_, "NN", "bf16", RESIDUAL, {}),                                                    # bwd qkv, joining the residual gradient
    (M_, H_, 3 * H_, "NN", "bf16", 0, {}),                                                           # bwd qkv
]


def split_parts(row, n1):
    """The two launches of a column split at n1: columns [0, n1) on 256-row tiles, the rest on 128-row tiles."""
    M, N, K, layout, out, flags, kw = row
    return [(M, n1, K, layout, out, flags, dict(kw, tile=256)), (M, N - n1, K, layout, out, flags, dict(kw, tile=128))]


def main():
    res = []
    for row in BASE_LAYER:
        p = plan(make_desc(*row[:6], **row[6]))
        parts = [plan(make_desc(*r[:6], **r[6])) for r in split_parts(row, p[5])] if p[5] else []
        res.append([list(p)] + [list(q) for q in parts])
    print("PLANS " + json.dumps(res))


if __name__ == "__main__":
    main()
