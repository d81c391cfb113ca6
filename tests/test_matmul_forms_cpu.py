"""hb_matmul_form, the host-side query of the GEMM's dispatch rules (no kernel runs here): its answers for the benchmark's
GEMM shapes and on both sides of every boundary of a rule, pinned as literals.  The literals were worked out by hand from
the rules as matmul_launch stated them before they moved into the decision function the launcher and the query share
(csrc/linalg.hip, matmul_decide) -- not by running the query.

One answer per case: (form, S, vec, finish, bfast, colsum_fused).  Operands are contiguous, 16-byte aligned, and the
workspace is matmul()'s (1 << 22 elements) unless the case says otherwise.

The rules, for reference.  rows (fp32): no transA, batch 1, M >= 2048, 8 <= K <= 256, K % 8 == 0, N <= 256, flags 0 or
ACTGRAD, beta 0, 32 NT WC (K + 4) <= 18432 LDS floats (NT WC = 8 for N > 128, 4 for N > 64, 2 for N > 32, else 1), A
aligned with lda % 4 == 0 (and B when transB); its register form when N > 32 and K in {16, 32, 64, 128}.  128-tiles:
M, N, K >= 256 and >= 200 active 128-tiles over the batch.  Split-K (64-tiles with a workspace): active tiles x batch
< 320 (or K >= 32768) and K >= 128; S = min((K >= 2048 ? 896 : 320) / tiles, K / 64, ws / (batch M N), 64), taken when
>= 2, rounded down to a multiple of 8 above 8.  In-workgroup split-K (fp32): the result would go through the workspace,
M % 32 == N % 32 == K % 128 == 0, 128 <= K <= 4096, at most 1024 32-tiles, aligned operands, no ACTGRAD.  Vector path:
aligned, leading dimensions and batch strides % (16 / elem) == 0, K % 16 == 0, the contiguous extent of each operand a
multiple of 16 / elem.  Batch-fastest grid: batch % 8 == 0."""
import pytest
import torch

from henbun_amd import hip_ops as H

F32, F64 = torch.float32, torch.float64
T64, T128, WGK, ROWS, RREG = 0, 1, 2, 3, 4


def _ans(dtype, batch, M, N, K, **kw):
    f = H.matmul_form(dtype, batch, M, N, K, **kw)
    return (f.form, f.S, int(f.vec), int(f.finish), int(f.bfast), int(f.colsum_fused))


PINNED = [
    # ---- the benchmark's GEMM shapes
    ('cfg2 512^3', (F32, 1, 512, 512, 512), {}, (WGK, 1, 0, 0, 0, 0)),
    ('cfg2 512^3 phi', (F32, 1, 512, 512, 512), {'flags': H.MM_PHI_OUT}, (WGK, 1, 0, 0, 0, 0)),
    ('cfg2 512^3 sym', (F32, 1, 512, 512, 512), {'flags': H.MM_SYM_OUT}, (WGK, 1, 0, 0, 0, 0)),
    ('cfg2 512^3 transA transB', (F32, 1, 512, 512, 512), {'transA': True, 'transB': True}, (WGK, 1, 0, 0, 0, 0)),
    ('cfg2 512^3 no workspace', (F32, 1, 512, 512, 512), {'ws_elems': 0}, (T64, 1, 1, 0, 0, 0)),
    ('cfg2 512^3 fp64', (F64, 1, 512, 512, 512), {}, (T64, 5, 1, 1, 0, 0)),
    ('cfg4 [32768,64]x[64,256]', (F32, 1, 32768, 256, 64), {}, (RREG, 1, 0, 0, 0, 0)),
    ('cfg4 [32768,256]x[256,32]', (F32, 1, 32768, 32, 256), {}, (ROWS, 1, 0, 0, 0, 0)),
    ('cfg4 [32768,256]x[256,64]^T actgrad', (F32, 1, 32768, 64, 256), {'transB': True, 'flags': H.MM_ACTGRAD}, (ROWS, 1, 0, 0, 0, 0)),
    ('cfg4 fp64 [32768,64]x[64,256]', (F64, 1, 32768, 256, 64), {}, (T64, 1, 1, 0, 0, 0)),
    ('cfg4 dW 64x256', (F32, 1, 64, 256, 32768), {'transA': True}, (T64, 64, 1, 1, 0, 0)),
    ('cfg4 dW 256x32', (F32, 1, 256, 32, 32768), {'transA': True}, (T64, 64, 1, 1, 0, 0)),
    ('cfg4 dW 16x64', (F32, 1, 16, 64, 32768), {'transA': True}, (T64, 64, 1, 1, 0, 0)),
    ('cfg4 dW+db 64x256', (F32, 1, 64, 256, 32768), {'transA': True, 'colsum': True}, (T64, 64, 1, 1, 0, 1)),
    ('cfg4 dW+db 256x32', (F32, 1, 256, 32, 32768), {'transA': True, 'colsum': True}, (T64, 64, 1, 1, 0, 1)),
    ('cfg4 dW+db 16x64', (F32, 1, 16, 64, 32768), {'transA': True, 'colsum': True}, (T64, 64, 1, 1, 0, 1)),
    ('cfg5 8x512^3', (F32, 8, 512, 512, 512), {}, (T64, 1, 1, 0, 1, 0)),
    ('cfg5 8x512^3 phi', (F32, 8, 512, 512, 512), {'flags': H.MM_PHI_OUT}, (T64, 1, 1, 0, 1, 0)),
    ('cfg5 8x512^3 sym', (F32, 8, 512, 512, 512), {'flags': H.MM_SYM_OUT}, (T64, 1, 1, 1, 1, 0)),
    # ---- in-workgroup split-K: K = 128 / 4096 / 4224, M % 32, 1024 tiles
    ('wgk K=64', (F32, 1, 64, 64, 64), {}, (T64, 1, 1, 0, 0, 0)),
    ('wgk K=128', (F32, 1, 64, 64, 128), {}, (WGK, 1, 0, 0, 0, 0)),
    ('wgk K=4096', (F32, 1, 64, 64, 4096), {}, (WGK, 1, 0, 0, 0, 0)),
    ('wgk K=4224', (F32, 1, 64, 64, 4224), {}, (T64, 64, 1, 1, 0, 0)),
    ('wgk M=48', (F32, 1, 48, 64, 128), {}, (T64, 2, 1, 1, 0, 0)),
    ('wgk N=48', (F32, 1, 64, 48, 128), {}, (T64, 2, 1, 1, 0, 0)),
    ('wgk 1024 tiles', (F32, 1, 1024, 1024, 128), {'flags': H.MM_SYM_OUT}, (WGK, 1, 0, 0, 0, 0)),
    ('wgk 1089 tiles', (F32, 1, 1056, 1056, 128), {'flags': H.MM_SYM_OUT}, (T64, 1, 1, 1, 0, 0)),
    ('wgk actgrad leaves', (F32, 1, 64, 64, 128), {'flags': H.MM_ACTGRAD}, (T64, 2, 1, 1, 0, 0)),
    ('wgk A misaligned', (F32, 1, 64, 64, 128), {'a_aligned': False}, (T64, 2, 0, 1, 0, 0)),
    ('wgk lda % 4', (F32, 1, 64, 64, 128), {'lda': 129}, (T64, 2, 0, 1, 0, 0)),
    ('wgk lda padded by 4', (F32, 1, 64, 64, 128), {'lda': 132, 'ldb': 68}, (WGK, 1, 0, 0, 0, 0)),
    ('wgk fp64 stays', (F64, 1, 64, 64, 128), {}, (T64, 2, 1, 1, 0, 0)),
    ('wgk colsum stays', (F32, 1, 64, 64, 128), {'transA': True, 'colsum': True}, (T64, 2, 1, 1, 0, 1)),
    # ---- row-streaming: M = 2047 / 2048, K = 256 / 264, K % 8, and what else it asks
    ('rows M=2047', (F32, 1, 2047, 64, 24), {}, (T64, 1, 0, 0, 0, 0)),
    ('rows M=2048', (F32, 1, 2048, 64, 24), {}, (ROWS, 1, 0, 0, 0, 0)),
    ('rows K=256', (F32, 1, 2048, 64, 256), {}, (ROWS, 1, 0, 0, 0, 0)),
    ('rows K=264', (F32, 1, 2048, 64, 264), {}, (T64, 4, 0, 1, 0, 0)),
    ('rows K=8', (F32, 1, 2048, 7, 8), {}, (ROWS, 1, 0, 0, 0, 0)),
    ('rows K=4', (F32, 1, 2048, 7, 4), {}, (T64, 1, 0, 0, 0, 0)),
    ('rows K=12', (F32, 1, 2048, 64, 12), {}, (T64, 1, 0, 0, 0, 0)),
    ('rows N=257', (F32, 1, 2048, 257, 64), {}, (T64, 1, 0, 0, 0, 0)),
    ('rows transA', (F32, 1, 2048, 64, 24), {'transA': True}, (T64, 1, 0, 0, 0, 0)),
    ('rows batch 2', (F32, 2, 2048, 64, 24), {}, (T64, 1, 0, 0, 0, 0)),
    ('rows beta', (F32, 1, 2048, 64, 24), {'beta': 2.0}, (T64, 1, 0, 0, 0, 0)),
    ('rows tril', (F32, 1, 2048, 64, 24), {'flags': H.MM_TRIL_OUT}, (T64, 1, 0, 0, 0, 0)),
    ('rows lda + 1', (F32, 1, 2048, 64, 24), {'lda': 25}, (T64, 1, 0, 0, 0, 0)),
    ('rows lda + 4', (F32, 1, 2048, 64, 24), {'lda': 28}, (ROWS, 1, 0, 0, 0, 0)),
    ('rows ldb + 1', (F32, 1, 2048, 64, 24), {'ldb': 65}, (ROWS, 1, 0, 0, 0, 0)),
    ('rows transB ldb + 1', (F32, 1, 2048, 64, 24), {'transB': True, 'ldb': 25}, (T64, 1, 0, 0, 0, 0)),
    ('rows A misaligned', (F32, 1, 2048, 64, 24), {'a_aligned': False}, (T64, 1, 0, 0, 0, 0)),
    ('rows B misaligned', (F32, 1, 2048, 64, 24), {'b_aligned': False}, (ROWS, 1, 0, 0, 0, 0)),
    ('rows transB B misaligned', (F32, 1, 2048, 64, 24), {'transB': True, 'b_aligned': False}, (T64, 1, 0, 0, 0, 0)),
    # ---- the rows LDS limit
    ('rows N=256 K=64', (F32, 1, 2048, 256, 64), {}, (RREG, 1, 0, 0, 0, 0)),
    ('rows N=256 K=72', (F32, 1, 2048, 256, 72), {}, (T64, 1, 0, 0, 0, 0)),
    ('rows N=128 K=136', (F32, 1, 2048, 128, 136), {}, (ROWS, 1, 0, 0, 0, 0)),
    ('rows N=128 K=144', (F32, 1, 2048, 128, 144), {}, (T64, 2, 1, 1, 0, 0)),
    ('rows N=129 K=64', (F32, 1, 2048, 129, 64), {}, (RREG, 1, 0, 0, 0, 0)),
    ('rows N=129 K=72', (F32, 1, 2048, 129, 72), {}, (T64, 1, 0, 0, 0, 0)),
    ('rows N=64 K=256', (F32, 1, 2048, 64, 256), {}, (ROWS, 1, 0, 0, 0, 0)),
    # ---- the register form: N = 32 / 33, K in {16, 32, 64, 128} against 24 / 96
    ('rowsreg N=32', (F32, 1, 2048, 32, 64), {}, (ROWS, 1, 0, 0, 0, 0)),
    ('rowsreg N=33', (F32, 1, 2048, 33, 64), {}, (RREG, 1, 0, 0, 0, 0)),
    ('rowsreg K=16', (F32, 1, 2048, 64, 16), {}, (RREG, 1, 0, 0, 0, 0)),
    ('rowsreg K=24', (F32, 1, 2048, 64, 24), {}, (ROWS, 1, 0, 0, 0, 0)),
    ('rowsreg K=32', (F32, 1, 2048, 64, 32), {}, (RREG, 1, 0, 0, 0, 0)),
    ('rowsreg K=64', (F32, 1, 2048, 64, 64), {}, (RREG, 1, 0, 0, 0, 0)),
    ('rowsreg K=96', (F32, 1, 2048, 64, 96), {}, (ROWS, 1, 0, 0, 0, 0)),
    ('rowsreg K=128', (F32, 1, 2048, 64, 128), {}, (RREG, 1, 0, 0, 0, 0)),
    ('rowsreg K=256', (F32, 1, 2048, 64, 256), {}, (ROWS, 1, 0, 0, 0, 0)),
    ('rowsreg actgrad', (F32, 1, 2048, 64, 64), {'flags': H.MM_ACTGRAD}, (RREG, 1, 0, 0, 0, 0)),
    # ---- 128-tiles: 200 active tiles over the batch.  (199 is prime and a matrix of 256 has at least three active
    # 128-tiles, so the nearest reachable counts are 196 / 200 with four tiles each and 198 / 201 with three.)
    ('bt 196 tiles', (F32, 49, 256, 256, 256), {}, (T64, 1, 1, 0, 0, 0)),
    ('bt 200 tiles', (F32, 50, 256, 256, 256), {}, (T128, 1, 1, 0, 0, 0)),
    ('bt 198 lower tiles', (F32, 66, 256, 256, 256), {'flags': H.MM_TRIL_OUT}, (T64, 1, 1, 0, 0, 0)),
    ('bt 201 lower tiles', (F32, 67, 256, 256, 256), {'flags': H.MM_TRIL_OUT}, (T128, 1, 1, 0, 0, 0)),
    ('bt 224 tiles batch fastest', (F32, 56, 256, 256, 256), {}, (T128, 1, 1, 0, 1, 0)),
    ('bt K=255', (F32, 50, 256, 256, 255), {}, (T64, 1, 0, 0, 0, 0)),
    ('bt M=255', (F32, 50, 255, 256, 256), {}, (T64, 1, 1, 0, 0, 0)),
    ('bt fp64 200 tiles', (F64, 50, 256, 256, 256), {}, (T128, 1, 1, 0, 0, 0)),
    # ---- the split rule: 319 / 320 tiles (K >= 2048, where 896 / 319 = 2 shows it), K = 127 / 128
    ('split 319 tiles', (F32, 319, 64, 64, 2048), {}, (T64, 2, 1, 1, 0, 0)),
    ('split 320 tiles', (F32, 320, 64, 64, 2048), {}, (T64, 1, 1, 0, 1, 0)),
    ('split K=127', (F32, 1, 48, 64, 127), {}, (T64, 1, 0, 0, 0, 0)),
    ('split K=128', (F32, 1, 48, 64, 128), {}, (T64, 2, 1, 1, 0, 0)),
    ('split K=144', (F32, 1, 64, 64, 144), {}, (T64, 2, 1, 1, 0, 0)),
    ('split workspace bound', (F32, 1, 48, 64, 1024), {'ws_elems': 3 * 48 * 64 + 5}, (T64, 3, 1, 1, 0, 0)),
    ('split workspace of one slab', (F32, 1, 48, 64, 1024), {'ws_elems': 48 * 64}, (T64, 1, 1, 0, 0, 0)),
    ('split K=32768 with many tiles', (F32, 8, 512, 512, 32768), {'ws_elems': 1 << 26}, (T64, 16, 1, 1, 1, 0)),
    # ---- S > 8 rounds down to a multiple of 8
    ('S 8 stays', (F32, 1, 48, 64, 512), {}, (T64, 8, 1, 1, 0, 0)),
    ('S 9 -> 8', (F32, 1, 48, 64, 576), {}, (T64, 8, 1, 1, 0, 0)),
    ('S 11 -> 8', (F32, 1, 64, 64, 704), {}, (T64, 8, 1, 1, 0, 0)),
    ('S 15 -> 8', (F32, 1, 48, 64, 960), {}, (T64, 8, 1, 1, 0, 0)),
    ('S 16 stays', (F32, 1, 48, 64, 1024), {}, (T64, 16, 1, 1, 0, 0)),
    ('S 64 transA vector', (F32, 1, 64, 64, 4112), {'transA': True}, (T64, 64, 1, 1, 0, 0)),
    ('S 64 scalar', (F32, 1, 7, 5, 4100), {}, (T64, 64, 0, 1, 0, 0)),
    ('S 64 fp64', (F64, 1, 64, 64, 4112), {'transA': True}, (T64, 64, 1, 1, 0, 0)),
    # ---- the vector path
    ('vec one step', (F32, 1, 64, 64, 16), {}, (T64, 1, 1, 0, 0, 0)),
    ('vec K=17', (F32, 1, 64, 64, 17), {}, (T64, 1, 0, 0, 0, 0)),
    ('vec N=130', (F32, 1, 65, 130, 16), {}, (T64, 1, 0, 0, 0, 0)),
    ('vec N=130 transB', (F32, 1, 65, 130, 16), {'transB': True}, (T64, 1, 1, 0, 0, 0)),
    ('vec M=65 transA', (F32, 1, 65, 132, 16), {'transA': True}, (T64, 1, 0, 0, 0, 0)),
    ('vec M=68 transA', (F32, 1, 68, 132, 16), {'transA': True}, (T64, 1, 1, 0, 0, 0)),
    ('vec fp64 N=2', (F64, 1, 2, 2, 16), {'transA': True}, (T64, 1, 1, 0, 0, 0)),
    ('vec fp64 N=3', (F64, 1, 2, 3, 16), {'transA': True}, (T64, 1, 0, 0, 0, 0)),
    ('vec A misaligned', (F32, 1, 64, 64, 16), {'a_aligned': False}, (T64, 1, 0, 0, 0, 0)),
    ('vec B misaligned', (F32, 1, 64, 64, 16), {'b_aligned': False}, (T64, 1, 0, 0, 0, 0)),
    ('vec lda + 1', (F32, 1, 64, 64, 16), {'lda': 17}, (T64, 1, 0, 0, 0, 0)),
    ('vec ldb + 1', (F32, 1, 64, 64, 16), {'ldb': 65}, (T64, 1, 0, 0, 0, 0)),
    ('vec lda, ldb + 4', (F32, 1, 64, 64, 16), {'lda': 20, 'ldb': 68}, (T64, 1, 1, 0, 0, 0)),
    ('vec fp64 lda + 1', (F64, 1, 64, 64, 16), {'lda': 17}, (T64, 1, 0, 0, 0, 0)),
    ('vec fp64 lda + 2', (F64, 1, 64, 64, 16), {'lda': 18}, (T64, 1, 1, 0, 0, 0)),
    ('vec sA + 1', (F32, 3, 64, 64, 16), {'sA': 64 * 16 + 1}, (T64, 1, 0, 0, 0, 0)),
    ('vec sA = 0', (F32, 3, 64, 64, 16), {'sA': 0}, (T64, 1, 1, 0, 0, 0)),
    # ---- the batch-fastest grid
    ('batch 3', (F32, 3, 68, 60, 48), {}, (T64, 1, 1, 0, 0, 0)),
    ('batch 8', (F32, 8, 68, 60, 48), {}, (T64, 1, 1, 0, 1, 0)),
    ('batch 16 fp64', (F64, 16, 68, 60, 48), {}, (T64, 1, 1, 0, 1, 0)),
    ('batch 8 wgk', (F32, 8, 128, 128, 384), {}, (WGK, 1, 0, 0, 0, 0)),
    # ---- column sums: fused on the vector path of the 64-tile A^T B form, else a reduction of their own
    ('colsum fused one slab', (F32, 1, 64, 64, 48), {'transA': True, 'colsum': True}, (T64, 1, 1, 0, 0, 1)),
    ('colsum K % 16', (F32, 1, 64, 64, 100), {'transA': True, 'colsum': True}, (T64, 1, 0, 0, 0, 0)),
    ('colsum N % 4', (F32, 1, 64, 30, 48), {'transA': True, 'colsum': True}, (T64, 1, 0, 0, 0, 0)),
    ('colsum empty slabs', (F32, 1, 64, 64, 4112), {'transA': True, 'colsum': True}, (T64, 64, 1, 1, 0, 1)),
    ('colsum 128-tiles', (F32, 1, 4096, 4096, 256), {'transA': True, 'colsum': True, 'ws_elems': 1 << 25}, (T128, 1, 1, 0, 0, 0)),
]
SWITCHED = [
    ('mm_no_wgk', 1, (F32, 1, 512, 512, 512), {}, (T64, 5, 1, 1, 0, 0)),
    ('mm_no_wgk', 1, (F32, 1, 512, 512, 512), {'flags': H.MM_PHI_OUT}, (T64, 8, 1, 1, 0, 0)),
    ('mm_no_wgk', 1, (F32, 8, 128, 128, 384), {}, (T64, 6, 1, 1, 1, 0)),
    ('mm_no_rows', 1, (F32, 1, 32768, 256, 64), {}, (T64, 1, 1, 0, 0, 0)),
    ('mm_no_rows', 1, (F32, 1, 32768, 32, 256), {}, (T64, 1, 1, 0, 0, 0)),
    ('mm_no_rowsreg', 1, (F32, 1, 32768, 256, 64), {}, (ROWS, 1, 0, 0, 0, 0)),
    ('mm_no_rowsreg', 1, (F32, 1, 32768, 32, 256), {}, (ROWS, 1, 0, 0, 0, 0)),
    ('mm_force_bt', 128, (F32, 1, 128, 128, 16), {}, (T128, 1, 1, 0, 0, 0)),
    ('mm_force_bt', 128, (F32, 1, 132, 260, 48), {}, (T128, 1, 1, 0, 0, 0)),
    ('mm_force_bt', 128, (F32, 1, 512, 512, 512), {}, (WGK, 1, 0, 0, 0, 0)),
    ('mm_force_bt', 64, (F32, 50, 256, 256, 256), {}, (T64, 1, 1, 0, 0, 0)),
    ('mm_force_s', 3, (F32, 1, 130, 130, 80), {}, (T64, 3, 0, 1, 0, 0)),
    ('mm_force_s', 3, (F32, 1, 130, 130, 80), {'ws_elems': 0}, (T64, 1, 0, 0, 0, 0)),
    ('mm_force_s', 20, (F32, 1, 48, 64, 1024), {}, (T64, 16, 1, 1, 0, 0)),
    ('mm_force_s', 20, (F32, 1, 48, 64, 64), {}, (T64, 4, 1, 1, 0, 0)),
    ('mm_force_s', 2, (F32, 1024, 32, 32, 128), {}, (WGK, 1, 0, 0, 0, 0)),
    ('mm_force_s', 2, (F32, 1025, 32, 32, 128), {}, (T64, 2, 1, 1, 0, 0)),
    ('mm_force_s', 4, (F32, 50, 256, 256, 256), {'ws_elems': 1 << 25}, (T128, 4, 1, 1, 0, 0)),
]


@pytest.fixture(autouse=True)
def _switches_cleared():
    H.debug_clear()
    yield
    H.debug_clear()


@pytest.mark.parametrize("name, args, kw, want", PINNED, ids=[p[0] for p in PINNED])
def test_form_of_benchmark_and_boundary_shapes(name, args, kw, want):
    assert _ans(*args, **kw) == want


@pytest.mark.parametrize("key, value, args, kw, want", SWITCHED,
                         ids=["%s=%d-%s" % (s[0], s[1], "x".join(str(v) for v in s[2][1:])) + ("-" + "-".join(s[3]) if s[3] else "")
                              for s in SWITCHED])
def test_form_with_each_switch_set(key, value, args, kw, want):
    H.debug_set(key, value)
    assert _ans(*args, **kw) == want


def test_enum_values_and_rejected_queries():
    assert H.MM_FORM == {"tile64": 0, "tile128": 1, "wgk": 2, "rows": 3, "rowsreg": 4}
    for bad in ((F32, 0, 64, 64, 16), (F32, 1, 0, 64, 16), (F32, 1, 64, 0, 16)):
        with pytest.raises(ValueError):
            H.matmul_form(*bad)
    with pytest.raises(ValueError):
        H.matmul_form(F32, 1, 64, 64, 16, lda=15)
    with pytest.raises(ValueError):
        H.matmul_form(F32, 1, 64, 64, 16, transA=True, colsum=True, ws_elems=128 * 64)
    # what matmul_launch rejects by extents, strides and flags (the two share matmul_reject_extents / _flags): the
    # accepted neighbour of each first, so that the rejection is the one named
    H.matmul_form(F32, 65535, 4, 4, 16)
    H.matmul_form(F32, 1, 1 << 20, 4, 2047)                               # M lda = 2^31 - 2^20
    H.matmul_form(F32, 1, 64, 64, 128, flags=H.MM_SYM_OUT, ws_elems=64 * 64)
    H.matmul_form(F32, 1, 64, 64, 128, flags=H.MM_SYMLOW_OUT)
    H.matmul_form(F32, 1, 64, 48, 128, flags=H.MM_ACTGRAD)
    H.matmul_form(F32, 1, 64, 64, 48, transA=True, colsum=True)
    H.matmul_form(F32, 32767, 16384, 16384, 16)                           # 65536 tiles x 32767 = 2^31 - 65536 workgroups
    for bad in (dict(args=(F32, 65536, 4, 4, 16)),                        # batch too large
                dict(args=(F32, 32768, 16384, 16384, 16)),                # 2^31 workgroups: grid too large
                dict(args=(F32, 1, 1 << 20, 4, 2048)),                    # M lda = 2^31: past 32-bit indexing
                dict(args=(F32, 1, 4, 1 << 20, 2048), transB=True),       # N ldb = 2^31
                dict(args=(F32, 1, 64, 64, 128), flags=H.MM_SYM_OUT, ws_elems=64 * 64 - 1),
                dict(args=(F32, 1, 64, 64, 128), flags=H.MM_SYM_OUT, ws_elems=0),
                dict(args=(F32, 1, 64, 48, 128), flags=H.MM_SYM_OUT),     # not square
                dict(args=(F32, 1, 64, 64, 128), flags=H.MM_SYM_OUT, beta=2.0),
                dict(args=(F32, 1, 64, 64, 128), flags=H.MM_SYM_OUT | H.MM_LOWER_OUT),
                dict(args=(F32, 1, 64, 48, 128), flags=H.MM_SYMLOW_OUT),
                dict(args=(F32, 1, 64, 64, 128), flags=H.MM_SYMLOW_OUT, beta=2.0),
                dict(args=(F32, 1, 64, 64, 128), flags=H.MM_SYMLOW_OUT | H.MM_PHI_OUT),
                dict(args=(F32, 1, 64, 48, 128), flags=H.MM_ACTGRAD, beta=2.0),
                dict(args=(F32, 1, 64, 48, 128), flags=H.MM_ACTGRAD | H.MM_LOWER_OUT),
                dict(args=(F32, 1, 64, 64, 48), colsum=True),             # hb_matmul_colsum is A^T B ...
                dict(args=(F32, 1, 64, 64, 48), transA=True, transB=True, colsum=True),
                dict(args=(F32, 1, 64, 64, 48), transA=True, ldb=68, colsum=True),      # ... over contiguous B ...
                dict(args=(F32, 2, 64, 64, 48), transA=True, colsum=True)):             # ... and not batched
        kw = dict(bad)
        args = kw.pop("args")
        with pytest.raises(ValueError):
            H.matmul_form(*args, **kw)


def test_wgk_form_agrees_with_the_shape_query_a_planner_asks():
    """hb_matmul_wgk_shape is the shape part of the WGK rule: for aligned contiguous operands and a result that goes
    through the workspace (SYM_OUT here), the two queries agree."""
    for M, K, batch in ((512, 512, 1), (1024, 128, 1), (1056, 128, 1), (512, 4096, 1), (64, 4224, 1), (64, 64, 1), (48, 128, 1)):
        f = H.matmul_form(F32, batch, M, M, K, flags=H.MM_SYM_OUT)
        assert (f.form == WGK) == H.matmul_wgk_shape(M, M, K, batch), (M, K, batch)
