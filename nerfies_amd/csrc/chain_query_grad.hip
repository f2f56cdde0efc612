// Kernels of a gradient query (nrf_query_points_grad / nrf_query_grid_grad, include/nerfies_amd.h): the density, its gradient with
// respect to the caller's point and the surface normal -grad / |grad|.
//   forward  (64-row tiles): chain_query.hip density_tile keeping what the reverse needs -- the posenc stash, the trunk's ReLU sign
//       words (nerf_chain.h fwd_tile<., STASH_BITS>'s images: 256 + 4 PKS bytes per row) and sigma'(raw), one float per row.  The
//       same pieces in the same order as density_tile: the same sigma bits.
//   reverse  (64-row tiles): nerf_chain.h bwd_tile started at the density.  ds = sigma'(raw) enters at the alpha head -- dpre_7 =
//       mask_7(ds (x) w_alpha) needs no GEMM; a use_alpha_condition model: d bn = ds (x) w_alpha[0:256], then the W_bn^T step -- and
//       runs down the trunk with the d-posenc section and its chain rule word for word (arithmetic and order).  No rgb logit^T,
//       rgb branch, per-ray sums, dY image or bias sum: nothing is accumulated across rows, so there is no atomic and a row's
//       gradient does not depend on the launch it ran in.
//   finish   (one thread per row): grad = J^T grad' through the warp Jacobian of the row (the existing primal + tangent + Jacobian
//       kernels of warp_chain.hip, launched as they are), and the normal.
// A translation unit of its own: every other chain kernel is compiled from unchanged text (profiles/field_gradient.md has the
// resource table before / after).  64-row tiles only, for the reason chain_query.hip gives.
#include "nerf_chain.h"

namespace nrf {

struct DensityGradFwdArgs1 { ChainFwdArgs a[1]; float* sigma; float* dsig; };   // a[]: read through a run-time index (nerf_chain.h ChainFwdArgs1)
struct DensityGradBwdArgs1 { ChainBwdArgs a[1]; const float* dsig; };

// chain_query.hip density_tile with the STASH_BITS stash; sigma (may be nullptr) [rows], dsig [ntiles * 64]
template <class G>
__device__ __forceinline__ void density_stash_tile(const ChainFwdArgs& A, float* __restrict__ sigma, float* __restrict__ dsig, const int tile,
                                                   const int T, float* smem, const int tid0, const int wave) {
  constexpr int ROWS = G::ROWS;
  float* act = smem;                  // [256][ROWS] swizzled
  float* pe = smem + TRUNK_W * ROWS;  // [max(PK, G::SCRATCH_ROWS)][ROWS]; reused as scratch after the skip layer
  const float* __restrict__ prm = A.params;
  const int PK = A.PK;
  const int PKS = (PK + 31) / 32 * 32;   // features per posenc stash tile (whole 32-feature blocks)
  const int nq_pe = PK / 16;
  int tid = tid0;
  asm volatile("" : "+v"(tid));   // per-tile lane constants (nerf_chain.h fwd_tile)
  const int lane = tid & 63;
  const int h = lane >> 5;
  const int p = G::prow(lane);
  const int part = G::part(wave, h);
  const int row0 = G::row0(tile, T);
  // ---- prologue: the point + SinusoidalEncoder (modules.py:213-228) ----
  {
    int r = row0 + p;
    r = r < A.rows ? r : A.rows - 1;
    const float x[3] = {A.points[3 * r], A.points[3 * r + 1], A.points[3 * r + 2]};
    auto put = [&](int k, float v) { pe[k * ROWS + p] = v; };
    if (part == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) put(c, x[c]);
    } else if (part == 1) {
      for (int k = A.P; k < PK; ++k) put(k, 0.f);
    }
    const float half_pi = 1.57079632679489661923f;   // fp32(pi/2), modules.py:222
    for (int f = part; f < A.F; f += G::PARTS) {
      const float fr = (float)(1 << f);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a = __fmul_rn(x[c], fr);
        put(3 + (2 * f) * 3 + c, sinf(a));
        put(3 + (2 * f + 1) * 3 + c, sinf(__fadd_rn(a, half_pi)));
      }
    }
  }
  __syncthreads();
  G::stash_posenc(pe, PK, PKS / 32, A.st_pe + (size_t)tile * PKS * TILE_ROWS, T, wave, lane);   // sin / cos of the reverse's chain rule

  f32x16 acc[G::RB][2];
  const float4* wpk4 = reinterpret_cast<const float4*>(A.wpk);
  const __amdgpu_buffer_rsrc_t no_stash = make_rsrc(nullptr, FRAG_TILE_256 * 4);
  // ---- trunk: 8 x Dense(256)+ReLU, skip concat [h, posenc] at layer A.skip (modules.py:41-50); the sign words stay ----
  const float4* wL0 = wpk4 + (A.pk.fwd_L[0] / 4) + wave * (PK / 4) * 64;
  WQuad<2> wnext = prefetch_quad<2>(wL0, lane);
  BiasRegs<2> bnext = bias_load<2>(prm + A.po.trunk_b[0], wave * 64, lane);
#pragma unroll 1
  for (int l = 0; l < TRUNK_DEPTH; ++l) {
    bias_set<2>(acc, bnext);
    if (l == 0) {
      G::template k_loop<2, false>(acc, pe, nq_pe, wL0, lane, wnext);
    } else {
      G::template k_loop<2, true>(acc, act, 16, wpk4 + (A.pk.fwd_L[l] / 4) + wave * 64 * 64, lane, wnext);
      if (l == A.skip) {
        const float4* w4b = wpk4 + (A.pk.fwd_L4b / 4) + wave * (PK / 4) * 64;
        G::template k_loop<2, false>(acc, pe, nq_pe, w4b, lane, prefetch_quad<2>(w4b, lane));
      }
    }
    wnext = prefetch_quad<2>(wpk4 + ((l + 1 < TRUNK_DEPTH ? A.pk.fwd_L[l + 1] : A.pk.fwd_bn) / 4) + wave * 64 * 64, lane);
    bnext = bias_load<2>(prm + (l + 1 < TRUNK_DEPTH ? A.po.trunk_b[l + 1] : A.po.bn_b), wave * 64, lane);
    __builtin_amdgcn_sched_barrier(0);
    fwd_epilogue<2, EPI_RELU, STASH_BITS, G>(acc, wave * 64, act, no_stash, 0,
                                             A.bits_trunk + (((size_t)l * A.ntiles + tile) * 4 + wave) * 128, lane, T);
  }
  // ---- use_alpha_condition: the head reads the bottleneck, Dense(256), no activation (modules.py:149-157) ----
  if (A.alpha_ct) {
    bias_set<2>(acc, bnext);
    G::template k_loop<2, true>(acc, act, 16, wpk4 + (A.pk.fwd_bn / 4) + wave * 64 * 64, lane, wnext);
    __builtin_amdgcn_sched_barrier(0);
    fwd_epilogue<2, EPI_LINEAR, STASH_NONE, G>(acc, wave * 64, act, no_stash, 0, nullptr, lane, T);
  }
  // ---- alpha head: four partial sums (wave w: the fmaf chain over k = 64 w .. 64 w + 63), combined in one order ----
  {
    const float4* __restrict__ wa4 = reinterpret_cast<const float4*>(prm + A.po.alpha_k) + wave * 16;
    float s = 0.f;
    const int k0 = wave * 64;
#pragma unroll 1
    for (int kc = 0; kc < 4; ++kc) {
      float4 w4[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) w4[i] = wa4[4 * kc + i];
      float a[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) a[i] = act[G::elem(k0 + 16 * kc + i, p)];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s = fmaf(a[4 * i], w4[i].x, s); s = fmaf(a[4 * i + 1], w4[i].y, s);
        s = fmaf(a[4 * i + 2], w4[i].z, s); s = fmaf(a[4 * i + 3], w4[i].w, s);
      }
    }
    if (G::part_writer(h)) pe[wave * ROWS + p] = s;   // scratch (the posenc is no longer needed for this tile)
    __syncthreads();
    if (part == 0) {
      float sigma_raw = (pe[p] + pe[ROWS + p]) + (pe[2 * ROWS + p] + pe[3 * ROWS + p]) + prm[A.po.alpha_b];
      if (A.alpha_ct) sigma_raw += A.alpha_ct[min((row0 + p) / A.S, A.B - 1)];
      const float sg = sigma_activation(sigma_raw, A.sigma_act);
      if (sigma && row0 + p < A.rows) sigma[(size_t)row0 + p] = sg;
      // sigma'(raw): softplus' = sigmoid(raw) = 1 - exp(-sigma) from the activated value (ray_kernels.hip composite_bwd), relu'
      dsig[(size_t)row0 + p] = A.sigma_act == 1 ? -expm1f(-sg) : (sg > 0.f ? 1.f : 0.f);
    }
    __syncthreads();   // scratch (aliases pe) is free again for the next tile's prologue
  }
}

__global__ __launch_bounds__(256, Tile64::WG_PER_CU) void nerf_density_stash_kernel(const DensityGradFwdArgs1 P) {
  const ChainFwdArgs& A = P.a[blockIdx.x >> 24];
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  int* tslot = reinterpret_cast<int*>(smem + ACT_FLOATS);   // posenc / scratch rows: free between tiles
  const TileIter ti = tile_iter(A.ntiles, A.k_old);
  for (int tile = A.tile_counter ? next_tile(A.tile_counter, tslot) : ti.first; tile < (A.tile_counter ? A.ntiles : ti.end);
       tile = A.tile_counter ? next_tile(A.tile_counter, tslot, tile) : tile + ti.step)
    density_stash_tile<Tile64>(A, P.sigma, P.dsig, tile, 0, smem, tid0, wave);
}

void launch_chain_density_stash(const ChainFwdArgs& a, float* sigma, float* dsig, int grid, hipStream_t stream) {
  DensityGradFwdArgs1 p;
  p.a[0] = a; p.sigma = sigma; p.dsig = dsig;
  const size_t lds = chain_fwd_lds_bytes<Tile64>(a.PK);
  (void)hipFuncSetAttribute((const void*)nerf_density_stash_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(nerf_density_stash_kernel, dim3(grid), dim3(256), lds, stream, p);
}

// One tile of the reverse chain from the density: nerf_chain.h bwd_tile<G, NoBwdAcc, false> from its alpha-head term on.  A reads
// params / po / wpk / pk / rows / ntiles / bits_trunk / d_points / st_pe / F / P / PK / skip / alpha_on_bn; dsig [ntiles * 64].
template <class G>
__device__ __forceinline__ void density_bwd_tile(const ChainBwdArgs& A, const float* __restrict__ dsig, const int tile, float* smem) {
  static_assert(G::FULL, "the d-points section is written for 64-row tiles");
  constexpr int ROWS = G::ROWS;
  constexpr int T = 0;
  float* act = smem;                    // [256][ROWS] swizzled: current dpre tile
  float* dr = smem + TRUNK_W * ROWS;    // [ROWS]: sigma'(raw) of the tile rows; then the d posenc tile [PK][ROWS]
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = G::row0(tile, T);
  const float* __restrict__ prm = A.params;
  const float4* wpk4 = reinterpret_cast<const float4*>(A.wpk);
  const __amdgpu_buffer_rsrc_t no_dy = make_rsrc(nullptr, FRAG_TILE_256 * 4);
  if (tid < ROWS) dr[tid] = dsig[(size_t)row0 + tid];
  // the first GEMM's weights: W_bn^T (use_alpha_condition) or W_7^T
  WQuad<2> wnext = prefetch_quad<2>(wpk4 + ((A.alpha_on_bn ? A.pk.bwd_bnT : A.pk.bwd_LT[TRUNK_DEPTH - 1]) / 4) + wave * 64 * 64, lane);
  __syncthreads();
  // ---- use_alpha_condition: the alpha head reads the bottleneck -- d bn = ds (x) w_alpha[0:256] on the VALU, linear ----
  if (A.alpha_on_bn) {
    int le = tid;
    asm volatile("" : "+v"(le));   // epilogue-local lane constants
    const int lane = le & 63, j = lane & 31;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const int n = wave * 64 + 32 * cb + j;
      (void)bwd_epilogue<G, false>([](int, int) { return make_float4(0.f, 0.f, 0.f, 0.f); }, true, dr, prm[A.po.alpha_k + n],
                                   [](const float4& v, int) { return v; }, 0.f, n, act, no_dy, 0, lane, T);
    }
    __syncthreads();
  }

  f32x16 acc[G::RB][2];
  // ---- l = 8, as bwd_tile's: d h8 = d bn . W_bn^T (use_alpha_condition) or, with no GEMM, ds (x) w_alpha ; mask h8 > 0 -> dpre_7 ----
  // ---- then l = 7..1:  d h_l = dpre_l . W_l[0:256]^T ; mask h_l > 0 -> dpre_{l-1} ----
  // Every step keeps bwd_tile's shape, the l = 8 one included, so that the d-posenc section below meets a skip layer at 7 as well.
#pragma unroll 1
  for (int l = TRUNK_DEPTH; l >= 1; --l) {
    // the output of this step is dpre_{l-1}; its mask is sign(pre_{l-1}) = bits_trunk[l-1]
    const auto mb = G::template mask_load<2>(A.bits_trunk + (((size_t)(l - 1) * A.ntiles + tile) * 4 + wave) * 128, lane);
    const bool head = l == TRUNK_DEPTH && !A.alpha_on_bn;   // the alpha head's own term: nothing to multiply
    zero_acc<2>(acc);
    if (!head) {
      const int woff = (l == TRUNK_DEPTH) ? A.pk.bwd_bnT : A.pk.bwd_LT[l];
      G::template k_loop<2, true>(acc, act, 16, wpk4 + (woff / 4) + wave * 64 * 64, lane, wnext);
    }
    wnext = prefetch_quad<2>(wpk4 + (A.pk.bwd_LT[l > 1 ? l - 1 : 1] / 4) + wave * 64 * 64, lane);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    {
      int le = tid;
      asm volatile("" : "+v"(le));   // epilogue-local lane constants: not live across the K loop
      const int lane = le & 63, j = lane & 31, h = lane >> 5;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const int n = wave * 64 + 32 * cb + j;
        const float wa = head ? prm[A.po.alpha_k + n] : 0.f;
        (void)bwd_epilogue<G, false>([&](int q, int) { return G::template piece<2>(acc, cb, q); }, head, dr, wa,
                                     [&](const float4& v, int q) { return mask4(v, G::template mask_nibble<2>(mb, cb, T, q, h)); }, 0.f, n, act,
                                     no_dy, 0, lane, T);
      }
    }
    __syncthreads();

    // ---- d posenc = dpre_skip . W_skip[256:]^T + dpre_0 . W0^T  (256 -> PK columns), nerf_chain.h bwd_tile.  Wave w owns
    //      MFMA row block w&1 (tile rows 2i + rb) x column block w>>1; the result goes to the dpe tile
    //      in LDS (aliases dr, dead since the l = 8 step), element (n, row) at n*64 + (row ^ (n & 31)) ----
    if (l - 1 == A.skip || l == 1) {
      float* dpe = dr;
      const bool first = (l - 1 == A.skip);
      int ln = lane;
      asm volatile("" : "+v"(ln));   // opaque: the per-lane constants of this section are recomputed here
      const float4* wq = wpk4 + ((first ? A.pk.bwd_L4bT : A.pk.bwd_L0T) / 4) + ln;
      const int rb = wave & 1, cb = wave >> 1;
      f32x16 a2;
#pragma unroll
      for (int r = 0; r < 16; ++r) a2[r] = 0.f;
      const int j = ln & 31, h = ln >> 5;
      const int i = j, kk = h;
      const int aoff = 2 * (i & 1) + rb;
      const int PKS = (A.PK + 31) / 32 * 32;
      const int npw = PKS / 32 * 2;   // pieces per wave: 2 or 4
      // B from L2 in batches of 4 float4, the next batch in flight under the current one's MFMAs
      auto load_b = [&](float4 (&b)[4], int bt) {
#pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = wq[(bt * 4 + u) * 64];
      };
      auto mma_b = [&](const float4 (&b)[4], int bt) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k0 = 4 * (bt * 4 + u) + kk;
          const float a0 = act[act_addr(k0, i >> 1) + aoff];
          const float a1 = act[act_addr(k0 + 2, i >> 1) + aoff];
          a2 = mfma32(a0, cb ? b[u].y : b[u].x, a2);
          a2 = mfma32(a1, cb ? b[u].w : b[u].z, a2);
        }
      };
      float4 b0[4], b1[4];
      load_b(b0, 0);
#pragma unroll 1
      for (int bt = 0; bt < 16; bt += 2) {
        load_b(b1, bt + 1);
        mma_b(b0, bt);
        if (bt + 2 < 16) load_b(b0, bt + 2);
        mma_b(b1, bt + 1);
      }
      const int n = 32 * cb + j;
      if (n < A.PK) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int row = 2 * c_row(reg, h) + rb;
          float* o = dpe + n * TILE_ROWS + (row ^ (n & 31));
          *o = first ? a2[reg] : *o + a2[reg];
        }
      }
      __syncthreads();
      if (!first) {
        // chain rule through SinusoidalEncoder: d sin(f x) = f cos(f x), d sin(f x + pi/2) = -f sin(f x),
        // with sin / cos taken from the forward posenc stash.  Every thread holds 4 rows of one feature per piece:
        // feature k's term  -+ 2^f * pe[k] * dpe[partner(k)]  goes to the contrib tile (act is dead), element (k, row)
        // at k*64 + (row ^ (k & 31)); 192 threads then sum their (row, c) over the 2F features in a fixed order.
        float* contrib = act;
        const int nfeat = 3 + 6 * A.F;
        float4 pv[4];
        {
          const float4* pe4 = reinterpret_cast<const float4*>(A.st_pe + (size_t)tile * PKS * TILE_ROWS) + ln;
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (u < npw) pv[u] = pe4[(wave + 4 * u) * 64];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (u < npw) {
            const int pid = wave + 4 * u, q = pid & 7;
            const int k = (pid >> 3) * 32 + j, g = (q & 1) + 2 * h + 4 * (q >> 1);
            if (k >= 3 && k < nfeat) {
              const int f = (k - 3) / 6, r = (k - 3) - 6 * f;
              const int partner = r < 3 ? k + 3 : k - 3;
              const float sgn = r < 3 ? -(float)(1 << f) : (float)(1 << f);
              const float* dp = dpe + partner * TILE_ROWS;
              float* co = contrib + k * TILE_ROWS;
              const float pvv[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w};
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int row = 4 * g + e;
                co[row ^ (k & 31)] = sgn * pvv[e] * dp[row ^ (partner & 31)];
              }
            }
          }
        }
        __syncthreads();
        if (tid < 3 * TILE_ROWS) {
          const int row = tid / 3, c = tid - 3 * row;
          float dx = dpe[c * TILE_ROWS + (row ^ c)];
          for (int f = 0; f < A.F; ++f) {
            const int ns = 3 + 6 * f + c, nc = ns + 3;
            dx += contrib[ns * TILE_ROWS + (row ^ (ns & 31))] + contrib[nc * TILE_ROWS + (row ^ (nc & 31))];
          }
          A.d_points[(size_t)tile * TILE_ROWS * 3 + tid] = dx;
        }
        __syncthreads();   // dr (aliased) and act are rewritten by the next tile
      }
    }
  }
}

__global__ __launch_bounds__(256, Tile64::WG_PER_CU) void nerf_density_bwd_kernel(const DensityGradBwdArgs1 P) {
  const ChainBwdArgs& A = P.a[blockIdx.x >> 24];
  extern __shared__ __attribute__((aligned(16))) float smem[];
#pragma unroll 1
  for (int tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) density_bwd_tile<Tile64>(A, P.dsig, tile, smem);
}

void launch_chain_density_bwd(const ChainBwdArgs& a, const float* dsig, int grid, hipStream_t stream) {
  DensityGradBwdArgs1 p;
  p.a[0] = a; p.dsig = dsig;
  const size_t lds = chain_lds_bytes<Tile64>(a.PK);
  (void)hipFuncSetAttribute((const void*)nerf_density_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(nerf_density_bwd_kernel, dim3(grid), dim3(256), lds, stream, p);
}

// grad = J^T grad' (jac: the warp Jacobian d x'_i / d x_j, row-major [rows][9]; nullptr: the identity) and the normal
//   s = fmaf(g.z, g.z, fmaf(g.y, g.y, g.x * g.x));  n = -(g * (1 / sqrtf(s)))  -- exactly 0 where s is 0 or not finite
// (include/nerfies_amd.h nrf_field_grad_out).  Either output may be nullptr.
__global__ void field_grad_finish_kernel(const float* __restrict__ d_points, const float* __restrict__ jac, int rows, float* __restrict__ grad,
                                         float* __restrict__ normals) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float* dp = d_points + 3 * (size_t)r;
  float g[3] = {dp[0], dp[1], dp[2]};
  if (jac) {
    const float* J = jac + 9 * (size_t)r;
    const float gp[3] = {g[0], g[1], g[2]};
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = fmaf(J[6 + c], gp[2], fmaf(J[3 + c], gp[1], __fmul_rn(J[c], gp[0])));
  }
  if (grad) {
#pragma unroll
    for (int c = 0; c < 3; ++c) grad[3 * (size_t)r + c] = g[c];
  }
  if (normals) {
    const float s = fmaf(g[2], g[2], fmaf(g[1], g[1], __fmul_rn(g[0], g[0])));
    const bool ok = s > 0.f && s < __builtin_inff();
    const float inv = ok ? 1.f / sqrtf(s) : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) normals[3 * (size_t)r + c] = ok ? -__fmul_rn(g[c], inv) : 0.f;
  }
}

void launch_field_grad_finish(const float* d_points, const float* jac, int rows, float* grad, float* normals, hipStream_t stream) {
  hipLaunchKernelGGL(field_grad_finish_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, d_points, jac, rows, grad, normals);
}

}  // namespace nrf
