// attn_prefix.h — shared-prefix decode attention for batched steps on a paged cache (option attn.shared_prefix; the groups: csrc/prefix_groups.h).
//
// Rows forked from one prompt (tgx_fork_row, tgx_beam_advance, n-best, one system prompt under many requests) name the SAME physical blocks for their first
// nb * 128 tokens.  attn_decode_mfma_kernel streams those blocks once per row, and its 32 query columns hold the G heads of ONE row (4 of 32 on Llama / Mistral).
// Here the shared blocks are streamed once per GROUP:
//   attn_prefix_mfma_kernel   grid (kv heads, splits, groups).  The 32 query columns hold head g of member row r at column r * G + g (up to 32 / G rows); a
//       workgroup takes a range of whole 128-token blocks of the shared run, its four waves walk their own 64-key blocks of it (K fragments straight from global
//       memory, V [key][d] in a wave-private LDS tile read by ds_read_b64_tr_b16, online softmax per column in registers: attn_decode_mfma.h's loop, no workgroup
//       barrier in it), meet once in LDS and leave ONE (o[hd], m, l) record per (row, head, split).  Every key of the range is a key of every member: no masking.
//       A 64-key block lies inside one page; its table entry is read through the group's first member row.
//   attn_tail_merge_kernel    grid (kv heads, rows): every row of the step, grouped or not.  The same loop over the row's own keys [nb * 128, pos] (nb = 0 for an
//       ungrouped row: its whole context) including the step's appended key, then the merge of the row's prefix records in split order with the four waves'
//       own, the softmax normalisation and the o_proj input (fp32 rows or 16-bit terms, act.round16 honoured) — what the direct form writes.
// No atomics, nothing depends on the order workgroups arrive in: the same bits run to run.  q is read from memory (the un-fused QKV finish, rope_kv_rows_kernel,
// ran before): three launches per layer where the fused matrix-core form has one — the price the option's threshold pays for.
//
// Roofline: HBM — 2 * kv_heads * hd * 2 bytes * (sum over groups of nb * 128 + sum over rows of their tails) per layer, against sum over rows of pos + 1.
// The plan table is data (prefix_groups::table): {nb, nsplit} per row, then {nb, nsplit, bps, n_rows, rows[32]} per group; unused groups read nsplit = 0 and exit.
#pragma once
#include "attn_decode_mfma.h"

namespace tgx {

constexpr int PFX_QCOLS = 32, PFX_SPLITS = 16, PFX_GROUP_INTS = 36, PFX_ROW_INTS = 2;      // == prefix_groups::QCOLS / MAX_SPLITS / GROUP_INTS / ROW_INTS

struct PrefixArgs {
  const float* q;            // [rows][heads][hd] fp32, RoPE applied
  long long q_stride;
  const void *k_cache, *v_cache;      // this layer's pools
  const int* blk_tbl;        // [rows][tbl_stride]
  long long tbl_stride;
  const int* plan;           // the plan table; groups from plan + rows_max * PFX_ROW_INTS
  int rows_max;
  float* rec;                // [rows][heads][PFX_SPLITS][hd + 4] prefix records
  const int* pos;            // tail kernel: keys [nb * 128, pos[row]] are the row's own
  float* out;                // [rows][heads * hd] fp32, or the 16-bit terms:
  unsigned short *out_hi, *out_lo;
  int heads, kv_heads, gfull, act16;
  float scale;
};

// the Q^T fragments of query column ql (B operand: 8 consecutive d at 16 kk + 8 hh) from an fp32 head vector, as hi / lo terms; qp == nullptr: a zero column
template <int DT, int HD>
__device__ __forceinline__ void pfx_q_frags(const float* qp, int hh, bf16x8 (&qh)[HD / 16], bf16x8 (&qlo)[HD / 16]) {
#pragma unroll
  for (int kk = 0; kk < HD / 16; kk++) {
    unsigned int wh[4] = {0u, 0u, 0u, 0u}, wl[4] = {0u, 0u, 0u, 0u};
    if (qp) {
      const f32x4* p = reinterpret_cast<const f32x4*>(qp + kk * 16 + 8 * hh);
      const f32x4 q0 = p[0], q1 = p[1];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        bf16_t h, l;
        split16<DT>(j < 4 ? q0[j] : q1[j - 4], h, l);
        if (j & 1) { wh[j >> 1] |= (unsigned int)h << 16; wl[j >> 1] |= (unsigned int)l << 16; }
        else { wh[j >> 1] = h; wl[j >> 1] = l; }
      }
    }
    qh[kk] = __builtin_bit_cast(bf16x8, u32x4{wh[0], wh[1], wh[2], wh[3]});
    qlo[kk] = __builtin_bit_cast(bf16x8, u32x4{wl[0], wl[1], wl[2], wl[3]});
  }
}

// One wave over the 64-key blocks blk0, blk0 + bstep, ... < blk_end of a paged row: S^T = K . Q^T, online softmax per query column (lane = column, the two half
// waves hold the two key halves), O^T += V^T . P^T.  n_keys: keys at and beyond it are masked (MASK) — every block walked holds a key below it.  sV: the wave's
// [64][HD + 32] V tile.  The arithmetic, term order and rescale rule are attn_decode_mfma_kernel's main loop
// (attn_decode_mfma.h, without its look-ahead and RAW prologue): a change to one loop belongs in the other.
template <int DT, int HD, bool MASK>
__device__ __forceinline__ void pfx_walk(const elem_t<DT>* kbase, const elem_t<DT>* vbase, const int* tbl, int kv_heads, int kvh, int blk0, int bstep, int blk_end, int n_keys,
                                         const bf16x8 (&qh)[HD / 16], const bf16x8 (&qlo)[HD / 16], float qs, bf16_t* sV, f32x16 (&oacc)[HD / 32], float& m_run, float& l_run) {
  typedef elem_t<DT> E;
  constexpr int LV = HD + 32, KS = HD / 16, NB = HD / 32, CH = HD / 8;
  const int lane = threadIdx.x & 63, hh = lane >> 5, ql = lane & 31;
  f32x16 zero16;
#pragma unroll
  for (int r = 0; r < 16; r++) zero16[r] = 0.f;
  for (int blk = blk0; blk < blk_end; blk += bstep) {     // wave-uniform trip count
    const int key0 = blk * 64, last = n_keys - 1 - key0;      // (>= 0)
    const size_t o0 = kv_paged_off(tbl, kv_heads, kvh, __builtin_amdgcn_readfirstlane(key0), HD);
    u32x4 vvr[CH], kfr[2][KS];
#pragma unroll
    for (int i = 0; i < CH; i++) {
      const int c = lane + 64 * i, row = c / CH, kc = c - row * CH;
      vvr[i] = *reinterpret_cast<const u32x4*>(vbase + o0 + (size_t)min(row, last) * HD + kc * 8);     // clamped inside the range; masked by P = 0
    }
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      const E* krow = kbase + o0 + (size_t)min(32 * sub + ql, last) * HD + 8 * hh;
#pragma unroll
      for (int kk = 0; kk < KS; kk++) kfr[sub][kk] = *reinterpret_cast<const u32x4*>(krow + kk * 16);
    }
    f32x16 sacc[2];
    float mx = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      const int kb = key0 + 32 * sub;
#pragma unroll
      for (int kk = 0; kk < KS; kk++) {
        const bf16x8 fk = __builtin_bit_cast(bf16x8, kfr[sub][kk]);
        sacc[sub] = mfma16<DT>(fk, qlo[kk], kk == 0 ? zero16 : sacc[sub]);
        sacc[sub] = mfma16<DT>(fk, qh[kk], sacc[sub]);
      }
      if (MASK && kb + 32 > n_keys) {      // the range ends inside (or before) this sub-tile
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int key = kb + (r & 3) + 8 * (r >> 2) + 4 * hh;
          if (key >= n_keys) sacc[sub][r] = -INFINITY;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; r++) mx = fmaxf(mx, sacc[sub][r]);
    }
#pragma unroll
    for (int i = 0; i < CH; i++) {
      const int c = lane + 64 * i, row = c / CH, kc = c - row * CH;
      *reinterpret_cast<u32x4*>(&sV[row * LV + kc * 8]) = vvr[i];
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * qs;
    const float m_new = fmaxf(m_run, mx);                 // finite: every block holds at least one key of the range
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    float sum = 0.f;
#pragma unroll
    for (int sub = 0; sub < 2; sub++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float p = __builtin_amdgcn_exp2f(fmaf(sacc[sub][r], qs, -m_new));   // exp2(-inf) = 0 for masked keys
        sacc[sub][r] = p;
        sum += p;
      }
    sum += __shfl_xor(sum, 32, 64);
    l_run = l_run * alpha + sum;
    m_run = m_new;
    if (__any(alpha != 1.f)) {
#pragma unroll
      for (int b = 0; b < NB; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) oacc[b][r] *= alpha;
    }
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
#pragma unroll
      for (int s2 = 0; s2 < 2; s2++) {
        unsigned int wh[4], wl[4];
        if constexpr (DT == DT_BF16) {
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const float p0 = sacc[sub][8 * s2 + 2 * j], p1 = sacc[sub][8 * s2 + 2 * j + 1];
            wh[j] = pack_bf16(p0, p1);
            wl[j] = pack_bf16(p0 - bf16_lo(wh[j]), p1 - bf16_hi(wh[j]));
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++) {
            bf16_t ph, pl;
            split16<DT>(sacc[sub][8 * s2 + j], ph, pl);
            if (j & 1) { wh[j >> 1] |= (unsigned int)ph << 16; wl[j >> 1] |= (unsigned int)pl << 16; }
            else { wh[j >> 1] = ph; wl[j >> 1] = pl; }
          }
        }
        const bf16x8 fph = __builtin_bit_cast(bf16x8, u32x4{wh[0], wh[1], wh[2], wh[3]});
        const bf16x8 fpl = __builtin_bit_cast(bf16x8, u32x4{wl[0], wl[1], wl[2], wl[3]});
        const int kloc = 32 * sub + 16 * s2 + 4 * hh;
#pragma unroll
        for (int b = 0; b < NB; b++) {
          const bf16_t* vblk = &sV[(kloc + ((lane & 15) >> 2)) * LV + 32 * b + (lane & 16) + 4 * (lane & 3)];
          const u32x2 v0 = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vblk)));
          const u32x2 v1 = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vblk + 8 * LV)));
          const bf16x8 fv = __builtin_bit_cast(bf16x8, u32x4{v0[0], v0[1], v1[0], v1[1]});
          oacc[b] = mfma16<DT>(fv, fpl, oacc[b]);
          oacc[b] = mfma16<DT>(fv, fph, oacc[b]);
        }
      }
    }
  }
}

// a wave's (o[HD], m, l) of query column ql into its LDS record (C/D layout of the 32x32 MFMA: row = (r & 3) + 8 (r >> 2) + 4 hh)
template <int HD>
__device__ __forceinline__ void pfx_store_rec(float* dst, const f32x16 (&oacc)[HD / 32], float m_run, float l_run, int hh) {
#pragma unroll
  for (int b = 0; b < HD / 32; b++)
#pragma unroll
    for (int r = 0; r < 16; r++) dst[32 * b + (r & 3) + 8 * (r >> 2) + 4 * hh] = oacc[b][r];
  if (hh == 0) { dst[HD] = m_run; dst[HD + 1] = l_run; }
}

template <int DT, int HD>
__global__ __launch_bounds__(256) void attn_prefix_mfma_kernel(const PrefixArgs a) {
  typedef elem_t<DT> E;
  constexpr int NW = 4, LV = HD + 32, NB = HD / 32, KS = HD / 16;
  constexpr float LOG2E = 1.4426950408889634f;
  extern __shared__ __attribute__((aligned(16))) bf16_t pfx_lds[];
  const int* grp = a.plan + (size_t)a.rows_max * PFX_ROW_INTS + (size_t)blockIdx.z * PFX_GROUP_INTS;
  const int nb = grp[0], nsplit = grp[1], bps = grp[2], n_rows = grp[3];
  const int kvh = blockIdx.x, sp = blockIdx.y;
  if (sp >= nsplit) return;                 // (workgroup-uniform: groups beyond the plan's read nsplit = 0)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, hh = lane >> 5, ql = lane & 31;
  const int G = a.gfull;
  const int mr = ql / G, mg = ql - mr * G;
  const bool qvalid = mr < n_rows;
  const int row = grp[4 + (qvalid ? mr : 0)];
  const int page1 = min(sp * bps + bps, nb);
  bf16x8 qh[KS], qlo[KS];
  pfx_q_frags<DT, HD>(qvalid ? a.q + row * a.q_stride + (size_t)(kvh * G + mg) * HD : nullptr, hh, qh, qlo);
  f32x16 oacc[NB];
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int r = 0; r < 16; r++) oacc[b][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  pfx_walk<DT, HD, false>(static_cast<const E*>(a.k_cache), static_cast<const E*>(a.v_cache), a.blk_tbl + grp[4] * a.tbl_stride, a.kv_heads, kvh, 2 * sp * bps + wv, NW, 2 * page1,
                          page1 * KV_BLOCK, qh, qlo, a.scale * LOG2E, pfx_lds + (size_t)wv * 64 * LV, oacc, m_run, l_run);
  // the four waves meet in LDS, merged in wave order: one record per (member row, head) and split
  __syncthreads();
  float* red = reinterpret_cast<float*>(pfx_lds);        // [NW][PFX_QCOLS][HD + 4]
  if (qvalid) pfx_store_rec<HD>(red + ((size_t)wv * PFX_QCOLS + ql) * (HD + 4), oacc, m_run, l_run, hh);
  __syncthreads();
  const int ncol = n_rows * G;
  for (int idx = tid; idx < ncol * HD; idx += 64 * NW) {
    const int col = idx / HD, d = idx - col * HD;
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; w++) M = fmaxf(M, red[((size_t)w * PFX_QCOLS + col) * (HD + 4) + HD]);
    float acc = 0.f, L = 0.f;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const float* rec = red + ((size_t)w * PFX_QCOLS + col) * (HD + 4);
      const float sw = (rec[HD] == -INFINITY) ? 0.f : exp2f(rec[HD] - M);      // a wave without a block of the range
      acc = fmaf(rec[d], sw, acc);
      L = fmaf(rec[HD + 1], sw, L);
    }
    const int r = col / G, g = col - r * G;
    float* out = a.rec + (((size_t)grp[4 + r] * a.heads + kvh * G + g) * PFX_SPLITS + sp) * (HD + 4);
    out[d] = acc;
    if (d == 0) { out[HD] = M; out[HD + 1] = L; }
  }
}

template <int DT, int HD>
__global__ __launch_bounds__(256) void attn_tail_merge_kernel(const PrefixArgs a) {
  typedef elem_t<DT> E;
  constexpr int NW = 4, LV = HD + 32, NB = HD / 32, KS = HD / 16;
  constexpr float LOG2E = 1.4426950408889634f;
  extern __shared__ __attribute__((aligned(16))) bf16_t pfx_lds[];
  const int kvh = blockIdx.x, row = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, hh = lane >> 5, ql = lane & 31;
  const int G = a.gfull;
  const int nb = a.plan[row * PFX_ROW_INTS], nsplit = a.plan[row * PFX_ROW_INTS + 1];
  const int n_keys = a.pos[row] + 1;        // > nb * 128: the host planned nb <= past / 128, and the step's own key is the row's (prefix_groups.h rule 2)
  const bool qvalid = ql < G;
  bf16x8 qh[KS], qlo[KS];
  pfx_q_frags<DT, HD>(qvalid ? a.q + row * a.q_stride + (size_t)(kvh * G + ql) * HD : nullptr, hh, qh, qlo);
  f32x16 oacc[NB];
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int r = 0; r < 16; r++) oacc[b][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  pfx_walk<DT, HD, true>(static_cast<const E*>(a.k_cache), static_cast<const E*>(a.v_cache), a.blk_tbl + row * a.tbl_stride, a.kv_heads, kvh, 2 * nb + wv, NW, (n_keys + 63) >> 6, n_keys,
                         qh, qlo, a.scale * LOG2E, pfx_lds + (size_t)wv * 64 * LV, oacc, m_run, l_run);
  __syncthreads();
  float* red = reinterpret_cast<float*>(pfx_lds);        // [NW][G][HD + 4]
  if (qvalid) pfx_store_rec<HD>(red + ((size_t)wv * G + ql) * (HD + 4), oacc, m_run, l_run, hh);
  __syncthreads();
  for (int idx = tid; idx < G * HD; idx += 64 * NW) {
    const int g = idx / HD, d = idx - g * HD;
    const float* pre = a.rec + ((size_t)row * a.heads + kvh * G + g) * PFX_SPLITS * (HD + 4);
    float M = -INFINITY;
    for (int s = 0; s < nsplit; s++) M = fmaxf(M, pre[(size_t)s * (HD + 4) + HD]);
#pragma unroll
    for (int w = 0; w < NW; w++) M = fmaxf(M, red[((size_t)w * G + g) * (HD + 4) + HD]);
    float acc = 0.f, L = 0.f;
    for (int s = 0; s < nsplit; s++) {        // the prefix records in split order (every one holds keys: m finite), then the waves' own
      const float* rec = pre + (size_t)s * (HD + 4);
      const float sw = exp2f(rec[HD] - M);
      acc = fmaf(rec[d], sw, acc);
      L = fmaf(rec[HD + 1], sw, L);
    }
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const float* rec = red + ((size_t)w * G + g) * (HD + 4);
      const float sw = (rec[HD] == -INFINITY) ? 0.f : exp2f(rec[HD] - M);
      acc = fmaf(rec[d], sw, acc);
      L = fmaf(rec[HD + 1], sw, L);
    }
    const size_t o = row * a.q_stride + (size_t)(kvh * G + g) * HD + d;      // (the row holds its own key: L > 0)
    if (a.out_hi) split16<DT>(acc / L, a.out_hi[o], a.out_lo[o]);
    else a.out[o] = round_storage_if<DT>(acc / L, a.act16);
  }
}

}  // namespace tgx
