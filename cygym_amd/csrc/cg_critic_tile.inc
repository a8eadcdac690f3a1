// cg_critic_tile.inc -- one tile of the critic behind layer 1: 16 candidates, row r of the tile on the lanes with lane % 16 == r.  The one
// text of it, included where a kernel scores candidates (coord_ascent_kernel, cg_coord_ascent.hpp; meta_kernel, cg_meta.hpp) -- not a
// function: the including kernels keep the registers and the schedule they have with the text in place.
// In scope at the point of inclusion:
//   p0, p1, p2   const float*: the three LDS rows whose sum ((p0 + p1) + p2) is the row's fc1 pre-activation, each advanced by 4 kk
//   w2l          const float4*: packed W2 in LDS, advanced by the lane
//   lds, pl      the LDS block and the kernel's plan: pl.b2 and pl.w3 are the offsets of b2 and w3
//   G1, nt2, r   H1 / 16, H2 / 16, lane % 16
// Leaves part[v] = sum over the H2 columns of w3 relu(h2 + b2) of tile row 4 kk + v, complete in all 16 lanes of the row group
// (before + b3).
  cg_floatx4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = cg_floatx4{0.f, 0.f, 0.f, 0.f};
  for (int g = 0; g < G1; ++g) {
    const float4 a0 = *reinterpret_cast<const float4*>(p0 + 16 * g), a1 = *reinterpret_cast<const float4*>(p1 + 16 * g),
                 a2 = *reinterpret_cast<const float4*>(p2 + 16 * g);
    float4 a = make_float4((a0.x + a1.x) + a2.x, (a0.y + a1.y) + a2.y, (a0.z + a1.z) + a2.z, (a0.w + a1.w) + a2.w);
    a.x = a.x > 0.f ? a.x : 0.f; a.y = a.y > 0.f ? a.y : 0.f; a.z = a.z > 0.f ? a.z : 0.f; a.w = a.w > 0.f ? a.w : 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (2 * p < nt2) {   // (uniform) output tiles 2 p and 2 p + 1 (an odd tile count: the last tile twice, its second copy unused)
        const int ta = 2 * p, tb = 2 * p + 1 < nt2 ? 2 * p + 1 : nt2 - 1;
        const float4 b0 = w2l[(size_t)(ta * G1 + g) * WAVE], b1 = w2l[(size_t)(tb * G1 + g) * WAVE];
        acc[2 * p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0.x, acc[2 * p], 0, 0, 0);
        acc[2 * p + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b1.x, acc[2 * p + 1], 0, 0, 0);
        acc[2 * p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b0.y, acc[2 * p], 0, 0, 0);
        acc[2 * p + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1.y, acc[2 * p + 1], 0, 0, 0);
        acc[2 * p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b0.z, acc[2 * p], 0, 0, 0);
        acc[2 * p + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b1.z, acc[2 * p + 1], 0, 0, 0);
        acc[2 * p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b0.w, acc[2 * p], 0, 0, 0);
        acc[2 * p + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b1.w, acc[2 * p + 1], 0, 0, 0);
      }
    }
  }
  // epilogue: D fragment = rows 4 kk + v, column 16 t2 + r  ->  Q(row) = b3 + sum over columns of w3 relu(. + b2)
  float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t2 = 0; t2 < 8; ++t2) {
    if (t2 < nt2) {
      const float bb = lds[pl.b2 + 16 * t2 + r], ww = lds[pl.w3 + 16 * t2 + r];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float h = acc[t2][v] + bb;
        part[v] += ww * (h > 0.f ? h : 0.f);
      }
    }
  }
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) {
#pragma unroll
    for (int v = 0; v < 4; ++v) part[v] += __shfl_xor(part[v], m);
  }
