"""The GEMM tile planner, pinned without a GPU: aptai_gemm_plan (the planner aptai_gemm_bf16 itself calls) against a literal table.

How the table was recorded.  Every expected value comes from the commit BEFORE the planner existed (b4bd80d, "Add forced alignment of
known transcripts"), never from the planner: that commit's aptai_gemm_bf16 was called on the very descriptors built here (make_desc) on a
machine without a GPU, where it validates, chooses the tile and then fails at the launch with status -2 and "<kernel name>: no ROCm-capable
device is detected" - the kernel name maps one to one onto the tile.  nbatch, nsplit, K-tiles per slab, the raster group and the column
cut of APTAI_GEMM_SPLITN=1 came from the same calls through two fprintf lines added to a scratch copy of that commit (just before its
launch ladder and in its column-split branch); the two parts of a column split were recorded by handing that commit the two
part-descriptors it builds itself.  Refusals are its status and aptai_last_error() text.  Knob rows ran in a process per setting.

STEP holds every distinct (M, N, K, layout, output type, flags, split_k, accumulate, batch, tile, out_pre, colscale_n) that reached
ops.gemm / ops.gemm_grouped (collected on an MI355X by wrapping ops._gemm_desc around one step of bench.py) in: one eager train step of
APTAI base at 16 x 10 s (aptai_base), one of Wav2Vec2_PR base at 16 x 10 s with its trainable conv stack (pr_base), one Force_APTAI
step (force), one eager APTAI large step at 8 x 10 s (aptai_large); * marks members of a grouped launch, planned here as single problems.
Expected tuples are (tile, nbatch, nsplit, K-tiles per slab, raster_gm, split column)."""
import json
import os
import subprocess
import sys

import pytest

from gemm_plan_child import (BASE_LAYER, BIAS, DGELU, DROPOUT, GELU, MUL_AUX, PRE_DGELU, RESIDUAL, RESIDUAL_F32,  # noqa: F401
                             make_desc, plan)

from aptai_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))

STEP = [
    ((4096, 512, 1024, "NT", "bf16", BIAS, dict()), (64, 1, 1, 16, 8, 0)),   # aptai_large
    ((4096, 1024, 512, "NT", "bf16", BIAS, dict()), (64, 1, 1, 8, 8, 0)),   # aptai_large
    ((4096, 1024, 1024, "NT", "bf16", BIAS | RESIDUAL | DROPOUT, dict()), (64, 1, 1, 16, 8, 0)),   # aptai_large
    ((4096, 1024, 4096, "NT", "bf16", BIAS | RESIDUAL | DROPOUT, dict()), (64, 1, 1, 64, 8, 0)),   # aptai_large
    ((4096, 3072, 1024, "NT", "bf16", BIAS, dict(colscale_n=1024)), (448, 1, 1, 16, 8, 0)),   # aptai_large
    ((4096, 4096, 1024, "NT", "bf16", BIAS | GELU | DROPOUT | PRE_DGELU, dict(out_pre=True)), (256, 1, 1, 16, 8, 0)),   # aptai_large
    ((8192, 512, 1024, "NT", "bf16", BIAS, dict()), (64, 1, 1, 16, 8, 0)),   # aptai_large
    ((8192, 512, 1024, "NT", "bf16", GELU, dict()), (64, 1, 1, 16, 8, 0)),   # aptai_base, force
    ((8192, 512, 1024, "NT", "bf16", GELU, dict(out_pre=True)), (64, 1, 1, 16, 8, 0)),   # pr_base
    ((8192, 768, 512, "NT", "bf16", BIAS, dict()), (192, 1, 1, 8, 8, 0)),   # aptai_base, pr_base, force
    ((8192, 768, 768, "NT", "bf16", BIAS | RESIDUAL | DROPOUT, dict()), (192, 1, 1, 12, 8, 0)),   # aptai_base, pr_base, force
    ((8192, 768, 3072, "NT", "bf16", BIAS | RESIDUAL | DROPOUT, dict()), (192, 1, 1, 48, 8, 0)),   # aptai_base, pr_base, force
    ((8192, 2304, 768, "NT", "bf16", BIAS, dict(colscale_n=768)), (192, 1, 1, 12, 8, 0)),   # aptai_base, pr_base, force
    ((8192, 3072, 768, "NT", "bf16", BIAS | GELU, dict()), (128, 1, 1, 12, 8, 0)),   # force
    ((8192, 3072, 768, "NT", "bf16", BIAS | GELU | DROPOUT, dict()), (128, 1, 1, 12, 8, 0)),   # force
    ((8192, 3072, 768, "NT", "bf16", BIAS | GELU | DROPOUT | PRE_DGELU, dict(out_pre=True)), (128, 1, 1, 12, 8, 0)),   # aptai_base, pr_base
    ((16384, 512, 1024, "NT", "bf16", GELU, dict()), (128, 1, 1, 16, 8, 0)),   # aptai_base, force
    ((16384, 512, 1024, "NT", "bf16", GELU, dict(out_pre=True)), (128, 1, 1, 16, 8, 0)),   # pr_base
    ((16384, 512, 1536, "NT", "bf16", BIAS, dict()), (128, 1, 1, 24, 8, 0)),   # aptai_large
    ((32768, 512, 1536, "NT", "bf16", BIAS, dict()), (256, 1, 1, 24, 8, 0)),   # aptai_large
    ((32768, 512, 1536, "NT", "bf16", GELU, dict()), (256, 1, 1, 24, 8, 0)),   # aptai_base, force
    ((32768, 512, 1536, "NT", "bf16", GELU, dict(out_pre=True)), (256, 1, 1, 24, 8, 0)),   # pr_base
    ((65536, 512, 1536, "NT", "bf16", BIAS, dict()), (256, 1, 1, 24, 8, 0)),   # aptai_large
    ((65536, 512, 1536, "NT", "bf16", GELU, dict()), (256, 1, 1, 24, 8, 0)),   # aptai_base, force
    ((65536, 512, 1536, "NT", "bf16", GELU, dict(out_pre=True)), (256, 1, 1, 24, 8, 0)),   # pr_base
    ((131072, 512, 1536, "NT", "bf16", BIAS, dict()), (256, 1, 1, 24, 8, 0)),   # aptai_large
    ((131072, 512, 1536, "NT", "bf16", GELU, dict()), (256, 1, 1, 24, 8, 0)),   # aptai_base, force
    ((131072, 512, 1536, "NT", "bf16", GELU, dict(out_pre=True)), (256, 1, 1, 24, 8, 0)),   # pr_base
    ((262144, 512, 1536, "NT", "bf16", GELU, dict()), (256, 1, 1, 24, 8, 0)),   # aptai_base, force
    ((262144, 512, 1536, "NT", "bf16", GELU, dict(out_pre=True)), (256, 1, 1, 24, 8, 0)),   # pr_base
    ((4096, 64, 1024, "NT", "f32", BIAS, dict()), (64, 1, 1, 16, 8, 0)),   # aptai_large
    ((8192, 64, 768, "NT", "f32", BIAS, dict()), (64, 1, 1, 12, 8, 0)),   # aptai_base, pr_base, force
    ((8192, 768, 768, "NT", "f32", BIAS | RESIDUAL_F32, dict(tile=128)), (128, 1, 1, 12, 8, 0)),   # force
    ((8192, 768, 3072, "NT", "f32", BIAS | RESIDUAL_F32, dict(tile=128)), (128, 1, 1, 48, 8, 0)),   # force
    ((4096, 512, 1024, "NN", "bf16", 0, dict()), (64, 1, 1, 16, 8, 0)),   # aptai_large
    ((4096, 1024, 64, "NN", "bf16", 0, dict()), (64, 1, 1, 1, 8, 0)),   # aptai_large
    ((4096, 1024, 1024, "NN", "bf16", 0, dict()), (64, 1, 1, 16, 8, 0)),   # aptai_large
    ((4096, 1024, 3072, "NN", "bf16", 0, dict()), (64, 1, 1, 48, 8, 0)),   # aptai_large
    ((4096, 1024, 4096, "NN", "bf16", 0, dict()), (64, 1, 1, 64, 8, 0)),   # aptai_large
    ((4096, 4096, 1024, "NN", "bf16", MUL_AUX, dict()), (256, 1, 1, 16, 8, 0)),   # aptai_large
    ((8192, 512, 768, "NN", "bf16", 0, dict()), (64, 1, 1, 12, 8, 0)),   # aptai_base, pr_base
    ((8192, 768, 64, "NN", "bf16", 0, dict()), (192, 1, 1, 1, 8, 0)),   # aptai_base, pr_base
    ((8192, 768, 768, "NN", "bf16", 0, dict()), (192, 1, 1, 12, 8, 0)),   # aptai_base, pr_base
    ((8192, 768, 2304, "NN", "bf16", RESIDUAL, dict()), (192, 1, 1, 36, 8, 0)),   # aptai_base, pr_base
    ((8192, 768, 3072, "NN", "bf16", RESIDUAL, dict()), (192, 1, 1, 48, 8, 0)),   # aptai_base, pr_base
    ((8192, 1024, 512, "NN", "bf16", DGELU, dict()), (128, 1, 1, 8, 8, 0)),   # pr_base
    ((8192, 3072, 768, "NN", "bf16", MUL_AUX, dict()), (128, 1, 1, 12, 8, 0)),   # aptai_base, pr_base
    ((16384, 1024, 512, "NN", "bf16", DGELU, dict()), (256, 1, 1, 8, 8, 0)),   # pr_base
    ((32768, 512, 512, "NN", "bf16", RESIDUAL | DGELU, dict()), (256, 1, 1, 8, 8, 0)),   # pr_base
    ((32768, 1024, 512, "NN", "bf16", DGELU, dict()), (256, 1, 1, 8, 8, 0)),   # pr_base
    ((65536, 512, 512, "NN", "bf16", RESIDUAL | DGELU, dict()), (256, 1, 1, 8, 8, 0)),   # pr_base
    ((65536, 1024, 512, "NN", "bf16", DGELU, dict()), (256, 1, 1, 8, 8, 0)),   # pr_base
    ((131072, 512, 512, "NN", "bf16", RESIDUAL | DGELU, dict()), (256, 1, 1, 8, 8, 0)),   # pr_base
    ((131072, 1024, 512, "NN", "bf16", DGELU, dict()), (256, 1, 1, 8, 8, 0)),   # pr_base
    ((262144, 512, 512, "NN", "bf16", RESIDUAL, dict()), (256, 1, 1, 8, 8, 0)),   # pr_base
    ((262144, 1024, 512, "NN", "bf16", 0, dict()), (256, 1, 1, 8, 8, 0)),   # pr_base
    ((8, 768, 8192, "TN", "f32", 0, dict()), (128, 1, 1, 128, 8, 0)),   # aptai_base*, pr_base*
    ((8, 1024, 4096, "TN", "f32", 0, dict()), (128, 1, 1, 64, 8, 0)),   # aptai_large*
    ((8, 2304, 8192, "TN", "f32", 0, dict()), (128, 1, 1, 128, 8, 0)),   # aptai_base*, pr_base*
    ((8, 3072, 4096, "TN", "f32", 0, dict()), (128, 1, 1, 64, 8, 0)),   # aptai_large*
    ((8, 3072, 8192, "TN", "f32", 0, dict()), (128, 1, 1, 128, 8, 0)),   # aptai_base*, pr_base*
    ((8, 4096, 4096, "TN", "f32", 0, dict()), (128, 1, 1, 64, 8, 0)),   # aptai_large*
    ((64, 768, 8192, "TN", "f32", 0, dict(split_k=8)), (128, 1, 8, 16, 8, 0)),   # aptai_base, pr_base
    ((64, 1024, 4096, "TN", "f32", 0, dict(split_k=4)), (128, 1, 4, 16, 8, 0)),   # aptai_large
    ((64, 8192, 4992, "TN", "f32", 0, dict(batch=(1, 16))), (128, 16, 1, 78, 8, 0)),   # aptai_large
    ((512, 1024, 8192, "TN", "f32", 0, dict(split_k=2)), (128, 1, 2, 64, 8, 0)),   # pr_base
    ((512, 1024, 16384, "TN", "f32", 0, dict(split_k=4)), (128, 1, 4, 64, 8, 0)),   # pr_base
    ((512, 1536, 32768, "TN", "f32", 0, dict(split_k=8)), (128, 1, 8, 64, 8, 0)),   # pr_base
    ((512, 1536, 65536, "TN", "f32", 0, dict(split_k=16)), (256, 1, 16, 64, 8, 0)),   # pr_base
    ((512, 1536, 131072, "TN", "f32", 0, dict(split_k=16)), (256, 1, 16, 128, 8, 0)),   # pr_base
    ((512, 1536, 262144, "TN", "f32", 0, dict(split_k=16)), (256, 1, 16, 256, 8, 0)),   # pr_base
    ((768, 512, 8192, "TN", "f32", 0, dict(split_k=4)), (128, 1, 4, 32, 8, 0)),   # aptai_base, pr_base
    ((768, 768, 8192, "TN", "f32", 0, dict()), (128, 1, 1, 128, 8, 0)),   # aptai_base*, pr_base*
    ((768, 3072, 8192, "TN", "f32", 0, dict()), (128, 1, 1, 128, 8, 0)),   # aptai_base*, pr_base*
    ((1024, 512, 4096, "TN", "f32", 0, dict(split_k=2)), (128, 1, 2, 32, 8, 0)),   # aptai_large
    ((1024, 1024, 4096, "TN", "f32", 0, dict()), (128, 1, 1, 64, 8, 0)),   # aptai_large*
    ((1024, 4096, 4096, "TN", "f32", 0, dict()), (128, 1, 1, 64, 8, 0)),   # aptai_large*
    ((2304, 768, 8192, "TN", "f32", 0, dict()), (128, 1, 1, 128, 8, 0)),   # aptai_base*, pr_base*
    ((3072, 768, 8192, "TN", "f32", 0, dict()), (128, 1, 1, 128, 8, 0)),   # aptai_base*, pr_base*
    ((3072, 1024, 4096, "TN", "f32", 0, dict()), (128, 1, 1, 64, 8, 0)),   # aptai_large*
    ((4096, 1024, 4096, "TN", "f32", 0, dict()), (128, 1, 1, 64, 8, 0)),   # aptai_large*
]

EXTRA = [
    # explicit tiles: 64-row tiles need a K-contiguous A (a K-major A runs as 128), the others pass through
    ((768, 768, 8192, "TN", "f32", 0, dict(tile=64)), (128, 1, 1, 128, 8, 0)),
    ((8192, 768, 768, "NT", "bf16", BIAS, dict(tile=64)), (64, 1, 1, 12, 8, 0)),
    ((8192, 768, 768, "NT", "bf16", BIAS, dict(tile=128)), (128, 1, 1, 12, 8, 0)),
    ((8192, 768, 768, "NT", "bf16", BIAS, dict(tile=192)), (192, 1, 1, 12, 8, 0)),
    ((8192, 768, 768, "NT", "bf16", BIAS, dict(tile=256)), (256, 1, 1, 12, 8, 0)),
    ((768, 3072, 8192, "TN", "f32", 0, dict(tile=192)), (192, 1, 1, 128, 8, 0)),
    ((768, 3072, 8192, "TN", "f32", 0, dict(tile=256)), (256, 1, 1, 128, 8, 0)),
    ((8192, 768, 768, "NT", "bf16", BIAS, dict(tile=448)), (448, 1, 1, 12, 8, 0)),
    ((8192, 768, 768, "NN", "bf16", 0, dict(tile=448)), (448, 1, 1, 12, 8, 0)),
    ((8192, 768, 768, "NT", "bf16", BIAS, dict(tile=257, sk=True)), (257, 1, 1, 12, 8, 0)),
    ((8192, 768, 3072, "NN", "f32", 0, dict(tile=257, sk=True)), (257, 1, 1, 48, 8, 0)),
    ((8192, 768, 768, "NT", "f32", BIAS | RESIDUAL_F32, dict(tile=64)), (64, 1, 1, 12, 8, 0)),
    # the rule's other outcomes and its edges
    ((8192, 8192, 8192, "NT", "bf16", 0, dict()), (256, 1, 1, 128, 8, 0)),
    ((4096, 4096, 1024, "NT", "bf16", BIAS, dict()), (256, 1, 1, 16, 8, 0)),
    ((2048, 2048, 1024, "NT", "bf16", 0, dict()), (64, 1, 1, 16, 8, 0)),
    ((4096, 3072, 1024, "NT", "bf16", BIAS | RESIDUAL, dict()), (448, 1, 1, 16, 8, 0)),
    ((4096, 3072, 1024, "NT", "bf16", BIAS | GELU, dict()), (256, 1, 1, 16, 8, 0)),
    ((4096, 3072, 960, "NT", "bf16", BIAS, dict()), (256, 1, 1, 15, 8, 0)),
    ((8192, 2304, 768, "NT", "bf16", BIAS, dict()), (192, 1, 1, 12, 8, 0)),
    ((8192, 2304, 768, "NT", "bf16", BIAS | DROPOUT, dict()), (64, 1, 1, 12, 8, 0)),
    ((8192, 2304, 1088, "NT", "bf16", BIAS, dict()), (64, 1, 1, 17, 8, 0)),
    ((8192, 768, 3072, "NT", "bf16", 0, dict()), (192, 1, 1, 48, 8, 0)),
    ((8192, 3072, 768, "NT", "bf16", 0, dict()), (128, 1, 1, 12, 8, 0)),
    ((8192, 3072, 768, "NT", "f32", 0, dict()), (128, 1, 1, 12, 8, 0)),
    ((128, 768, 768, "NT", "bf16", BIAS, dict()), (64, 1, 1, 12, 8, 0)),
    ((64, 768, 768, "NT", "bf16", BIAS, dict()), (128, 1, 1, 12, 8, 0)),
    ((192, 3072, 768, "NT", "bf16", 0, dict()), (128, 1, 1, 12, 8, 0)),
    ((8192, 128, 768, "NT", "bf16", BIAS, dict()), (64, 1, 1, 12, 8, 0)),
    ((8192, 8, 768, "NT", "bf16", 0, dict()), (64, 1, 1, 12, 8, 0)),
    ((8192, 8, 768, "NN", "f32", 0, dict()), (64, 1, 1, 12, 8, 0)),
    ((8, 8, 64, "TN", "f32", 0, dict()), (128, 1, 1, 1, 8, 0)),
    ((8200, 776, 768, "NT", "bf16", 0, dict()), (128, 1, 1, 12, 8, 0)),
    ((512, 512, 64, "NT", "bf16", 0, dict(batch=(16, 12))), (256, 192, 1, 1, 8, 0)),
    ((512, 512, 64, "NN", "bf16", 0, dict(batch=(16, 12))), (256, 192, 1, 1, 8, 0)),
    ((512, 64, 512, "NT", "f32", 0, dict(batch=(192, 1))), (64, 192, 1, 8, 8, 0)),
    ((48, 48, 6144, "TN", "f32", 0, dict(batch=(1, 16))), (128, 16, 1, 96, 8, 0)),
    ((768, 768, 256, "TN", "f32", 0, dict(split_k=16)), (128, 1, 4, 1, 8, 0)),
    ((768, 768, 320, "TN", "f32", 0, dict(split_k=4)), (128, 1, 3, 2, 8, 0)),
    ((768, 768, 8192, "TN", "f32", 0, dict(split_k=4, accumulate=True)), (128, 1, 4, 32, 8, 0)),
    ((768, 768, 8192, "TN", "f32", 0, dict(accumulate=True)), (128, 1, 1, 128, 8, 0)),
    ((768, 3072, 8192, "TN", "f32", 0, dict(split_k=2)), (128, 1, 2, 64, 8, 0)),
]

REFUSALS = [
    # stream-K without its workspace
    ((8192, 768, 768, "NT", "bf16", BIAS, dict(tile=257)), -1,
     'aptai_gemm_bf16: tile 257 (stream-K) needs sk_workspace (aptai_gemm_sk_workspace_bytes), no batching / split-K / accumulate and M, N >= 256'),
    # ... below one 256 x 256 tile
    ((128, 768, 768, "NT", "bf16", BIAS, dict(tile=257, sk=True)), -1,
     'aptai_gemm_bf16: tile 257 (stream-K) needs sk_workspace (aptai_gemm_sk_workspace_bytes), no batching / split-K / accumulate and M, N >= 256'),
    # 256 x 192 tiles with fp32 output
    ((8192, 768, 768, "NT", "f32", 0, dict(tile=448)), -1,
     'aptai_gemm_bf16: tile 448 (256 x 192) is built for bf16 output, K-contiguous A, no batching / split-K'),
    ((768, 768, 8192, "TN", "f32", 0, dict(tile=448)), -1,
     'aptai_gemm_bf16: tile 448 (256 x 192) is built for bf16 output, K-contiguous A, no batching / split-K'),
    # fp32 residual under the auto rule
    ((8192, 768, 768, "NT", "f32", BIAS | RESIDUAL_F32, dict()), -1,
     'aptai_gemm_bf16: EPI_RESIDUAL_F32 needs fp32 output, a residual, no split-K / accumulate and an explicit tile'),
    # K not a multiple of 64
    ((8192, 768, 100, "NT", "bf16", 0, dict()), -1,
     'aptai_gemm_bf16: K=100 must be a multiple of 64'),
    # N not a multiple of 8
    ((8192, 772, 768, "NT", "bf16", 0, dict()), -1,
     'aptai_gemm_bf16: N=772 must be a multiple of 8'),
    # A K-major with B K-contiguous
    ((768, 768, 8192, "TT", "f32", 0, dict()), -1,
     'aptai_gemm_bf16: A K-major with B K-contiguous is not built'),
    ((768, 768, 8192, "TT", "f32", 0, dict(tile=256)), -1,
     'aptai_gemm_bf16: A K-major with B K-contiguous is not built'),
    # split-K with bf16 output
    ((768, 768, 8192, "TN", "bf16", 0, dict(split_k=4)), -1,
     'aptai_gemm_bf16: split-K needs fp32 output'),
    ((768, 768, 8192, "TN", "f32", 0, dict(split_k=4, workspace=False)), -1,
     'aptai_gemm_bf16: split-K / accumulate needs a workspace'),
    ((512, 512, 64, "NT", "f32", 0, dict(batch=(16, 12), accumulate=True)), -1,
     'aptai_gemm_bf16: batched GEMM cannot split-K/accumulate'),
    ((8192, 768, 768, "NT", "bf16", BIAS, dict(colscale_n=772)), -1,
     'aptai_gemm_bf16: colscale_n must be a multiple of 8 within N, bf16 output only'),
    ((0, 768, 768, "NT", "bf16", 0, dict()), -1,
     'aptai_gemm_bf16: empty problem M=0 N=768 K=768'),
]

KNOBS = [
    ({"APTAI_GEMM_TILE": "128"},
     [[(128, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 48, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 48, 8, 0)],
      [(128, 1, 1, 48, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 36, 8, 0)],
      [(128, 1, 1, 36, 8, 0)]]),
    ({"APTAI_GEMM_M64": "0"},
     [[(192, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 48, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 48, 8, 0)],
      [(192, 1, 1, 48, 8, 0)],
      [(192, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 36, 8, 0)],
      [(192, 1, 1, 36, 8, 0)]]),
    ({"APTAI_GEMM_M64": "2"},
     [[(192, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 48, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 48, 8, 0)],
      [(192, 1, 1, 48, 8, 0)],
      [(192, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 36, 8, 0)],
      [(192, 1, 1, 36, 8, 0)]]),
    ({"APTAI_GEMM_F256": "1.0"},
     [[(192, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 48, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 48, 8, 0)],
      [(192, 1, 1, 48, 8, 0)],
      [(192, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 36, 8, 0)],
      [(192, 1, 1, 36, 8, 0)]]),
    ({"APTAI_GEMM_RASTER": "0"},
     [[(192, 1, 1, 12, 0, 0)],
      [(192, 1, 1, 12, 0, 0)],
      [(128, 1, 1, 12, 0, 0)],
      [(192, 1, 1, 48, 0, 0)],
      [(128, 1, 1, 12, 0, 0)],
      [(192, 1, 1, 48, 0, 0)],
      [(192, 1, 1, 48, 0, 0)],
      [(192, 1, 1, 12, 0, 0)],
      [(192, 1, 1, 36, 0, 0)],
      [(192, 1, 1, 36, 0, 0)]]),
    ({"APTAI_GEMM_SPLITN": "1"},
     [[(192, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 12, 8, 0)],
      [(256, 1, 1, 12, 8, 2048), (256, 1, 1, 12, 8, 0), (128, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 48, 8, 0)],
      [(256, 1, 1, 12, 8, 2048), (256, 1, 1, 12, 8, 0), (128, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 48, 8, 0)],
      [(192, 1, 1, 48, 8, 0)],
      [(192, 1, 1, 12, 8, 0)],
      [(192, 1, 1, 36, 8, 0)],
      [(192, 1, 1, 36, 8, 0)]]),
    ({"APTAI_GEMM_SPLITN": "1", "APTAI_GEMM_TILE": "128"},
     [[(128, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 48, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 48, 8, 0)],
      [(128, 1, 1, 48, 8, 0)],
      [(128, 1, 1, 12, 8, 0)],
      [(128, 1, 1, 36, 8, 0)],
      [(128, 1, 1, 36, 8, 0)]]),
]


def _id(row):
    M, N, K, layout, out, flags, kw = row
    return f"{M}x{N}x{K}-{layout}-{out}-f{flags}" + "".join(f"-{k}{v}" for k, v in sorted(kw.items()))


@pytest.mark.parametrize("row,expected", STEP + EXTRA, ids=[_id(r) for r, _ in STEP + EXTRA])
def test_plan_matches_the_recorded_launch(row, expected):
    assert plan(make_desc(*row[:6], **row[6])) == expected


def test_the_table_reaches_every_kernel():
    assert {e[0] for _, e in STEP + EXTRA} == {64, 128, 192, 256, 448, 257}
    assert {e[0] for _, e in STEP} >= {64, 128, 192, 256, 448}          # the rule's own outcomes, without an explicit tile


@pytest.mark.parametrize("row,status,text", REFUSALS, ids=[_id(r) for r, _, _ in REFUSALS])
def test_refusals_keep_status_and_text(row, status, text):
    with pytest.raises(_lib.AptaiHipError) as e:
        plan(make_desc(*row[:6], **row[6]))
    assert str(e.value) == f"aptai_gemm_plan failed (status {status}): {text}"


@pytest.mark.parametrize("env,expected", KNOBS, ids=["+".join(f"{k[11:]}={v}" for k, v in sorted(e.items())) for e, _ in KNOBS])
def test_knobs_in_a_process_of_their_own(env, expected):
    clean = {k: v for k, v in os.environ.items() if not k.startswith(("APTAI_GEMM_", "APTAI_EPI_"))}
    r = subprocess.run([sys.executable, os.path.join(HERE, "gemm_plan_child.py")], env=dict(clean, **env), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PLANS ")][-1]
    got = [[tuple(p) for p in shape] for shape in json.loads(line[6:])]
    assert got == expected
    if env == {"APTAI_GEMM_SPLITN": "1"}:                 # 8192 x 3072: columns [0, 2048) on 256-row tiles, the rest on 128-row tiles
        for i, row in enumerate(BASE_LAYER):
            if row[1] == 3072:
                assert [p[0] for p in got[i]] == [256, 256, 128] and got[i][0][5] == 2048
    if "APTAI_GEMM_TILE" in env:
        assert all(len(shape) == 1 and shape[0][5] == 0 for shape in got)
