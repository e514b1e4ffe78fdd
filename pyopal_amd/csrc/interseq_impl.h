// Inter-sequence DP kernel for gfx950: scores of one query against 128 targets
// per wavefront, for all four alignment modes. Included by the interseq_*.hip
// translation units, one per arithmetic flavour (keeps hipcc builds parallel).
//
// Replaces the SIMD inner loop of opalSearchDatabase (declared
// src/pyopal/opal.pxd:38-52; the SSE/AVX2 body lives in the absent
// vendor/opal) for searchType = OPAL_SEARCH_SCORE.
//
// Mapping. SWIPE's "one SIMD lane = one database sequence" is widened to the
// 64-lane wavefront, and every lane carries TWO targets in the halves of a
// 32-bit VGPR (packed 16-bit arithmetic), so a wavefront advances 128 targets
// by one database column per pass over the query rows. The query rows of a
// strip (R <= 64) live in registers as H[R], E[R]; the substitution scores of
// the strip ("query profile", one row per residue symbol) live in LDS and are
// fetched with one ds_read_b128 per 8 rows per target.
//
// Long queries are cut into strips of R rows. The W wavefronts of a workgroup
// work on the SAME 128 targets, wavefront w on strip w of the current round,
// one 4-column chunk behind wavefront w-1 (a software pipeline along the
// anti-diagonal of (strip, chunk)); the last row of a strip reaches the next
// strip through a 2 KB LDS buffer, and only the hop from strip W-1 to strip 0 of
// the next round goes through HBM, in [column][lane] order (512 B per
// wavefront-column, coalesced). With W = 1 this degenerates to one wavefront per
// group walking its strips in turn.
//
// Cell update, per pair of targets:
//   h    = max(Hdiag + s, E[r], F)
//   hmo  = h - open
//   E[r] = max(E[r] - ext, hmo)        (gap consuming target residues)
//   F    = max(F - ext, hmo)           (gap consuming query residues)
// Arithmetic flavours (struct Arith*):
//   ArithSwF16  Smith-Waterman, packed half floats (integers exact below 2048);
//               E and F are floored at 0, so H needs no floor of its own, and
//               v_pk_maximum3_f16 folds two max per cell: 7.5 ops + 1 v_perm.
//   ArithSwI16  Smith-Waterman, saturating int16 with unsigned-saturating
//               subtraction for the same floor: 9 ops + 1 v_perm.
//   ArithI16    signed saturating int16 for NW / HW / OV and for the anchored
//               reverse pass: 8 ops + 1 v_perm (+1 when every cell is a candidate).
// A lane that reaches the limit of its flavour is flagged; the host recomputes
// it with the next rung (int16, then the int32 intra-sequence kernel): the
// reference's 8/16/32-bit ladder (src/pyopal/lib.pyx:1283-1289) on hardware that
// has no packed 8-bit max. (ds_read_u16_d16[_hi] cannot build the {A, B} score
// pair for free: with SRAM-ECC registers gfx950 d16 loads overwrite the whole
// VGPR; measured.)
//
// The kernels live in one header per family; this file is what the translation units include:
//   interseq_pair_parts.h          what the pair-table kernels share: the representation's constants, the
//                                  compile-time knobs, the table's layout and row address, the boundary rows
//                                  between strips, the pacing of a SIMD's wavefronts, the priority step
//   interseq_pair_table_build.inc  the table build, interseq_pair_handout.inc the group hand-out of the one-strip
//   interseq_strip_frame.inc       kernels, and the unit frame of the multi-strip kernels: each written once and
//                                  included as text by the kernels that have it (functions changed the code objects)
//   interseq_packed_ops.h          packed 16-bit operations on register halves (all families)
//   interseq_general.h             the general kernel and its arithmetic flavours, interseq_pair_kernel
//   interseq_pair_sw.h             one-strip Smith-Waterman on the pair table, with the column split
//   interseq_pair_sw_strips.h      Smith-Waterman of several strips
//   interseq_pair_global.h         one-strip NW / HW / OV
//   interseq_pair_global_strips.h  NW / HW / OV of several strips
#pragma once
#include "interseq_packed_ops.h"
#include "interseq_pair_parts.h"
#include "interseq_general.h"
#include "interseq_pair_sw.h"
#include "interseq_pair_sw_strips.h"
#include "interseq_pair_global.h"
#include "interseq_pair_global_strips.h"
