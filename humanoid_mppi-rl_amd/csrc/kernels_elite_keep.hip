// Keep / shift elites (mppi_set_elite_keep; the rule is elite_keep.h):
//   v[b][u][t][j] = the control sample idx[j] applied at step t + shift          keep_gather_kernel, behind the selection
//                   (+ kcost, idx, count, steps of the stored set)               and ahead of the lambda search / reduce
//   eps[b][u][t][j] = v[b][u][t][j] - U[b][u][t]   j < count[b], t < steps[b]    keep_inject_kernel, in place over the
//                                                                                next solve's noise ahead of its rollout
// Both work on the noise buffer beside the rollout and reduce kernels, never inside them: a solve with the feature on is
// routed exactly as without it.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "elite_keep.h"
#include "mppi_internal.h"

namespace mppi {

// ------------------------------------------------------------------------------------------------
// Ownership, both kernels: the solve's noise is B solves of RB = nu H rows of Kp floats (k fastest); the stored set is
// the same rows at `pitch` = n_keep rounded up to 4 floats (j fastest; the rows stay 16-B aligned).  A WAVE owns
// (b, a tile of T consecutive (u, t) rows of that b) and, in the gather, ONE 64-column stride of the set (j = lane +
// 64 stride; waves numbered stride-fastest, so the four waves of a block walk the same rows); the inject's wave loops
// over its strides of 16-B quads.  A lane loads its idx[j] once and walks the tile's rows with all T loads issued
// before the first is consumed; U is wave-uniform (scalar loads).  idx is ascending, so a wave's lanes read ascending
// addresses of one 4 Kp-byte noise row -- every 128-B line of the solve's noise is requested by at most one wave
// instruction per row and stride -- and store 256 contiguous bytes per row.  (One j per lane keeps the stores
// contiguous across the wave; four j per lane would make each lane's store 16 B and its four loads four scattered
// addresses: the loads bound the kernel, not the stores.)  T is chosen by the launcher so that small solves still
// spread over the chip.  No atomics, no LDS, nothing to zero.
// Two other forms of the gather were built, measured on config #4 at n_keep = K / 8 and removed:
// one wave looping over all strides of its tile (half as many waves, each twice as long), and a streaming form that
// read every row whole, 16 B per lane, into a wave-private LDS row and gathered from LDS.
// ------------------------------------------------------------------------------------------------

// The gather.  Rows t >= steps and columns j >= m (the pitch's pads included) store +0.0; lanes with j >= pitch store
// nothing.  The wave of tile 0 and stride 0 also writes the set's kcost, idx, count and steps.  An index outside [0, K) is never
// dereferenced (the selection writes none; the check keeps a stale buffer from becoming an address).
template <int T>
__global__ __launch_bounds__(256) void keep_gather_kernel(KeepArgs a, int shift, int tpb, int ns, int nwave) {
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (int)blockIdx.x * 4;
  if (w >= nwave) return;  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const int wt = (int)((unsigned)w / (unsigned)ns), stride = w - wt * ns;  // (stride fastest: a block's waves share rows)
  const int b = (int)((unsigned)wt / (unsigned)tpb), tile = wt - b * tpb;
  const int RB = a.nu * a.H, r0 = tile * T;
  const int sh = shift ? 1 : 0, steps = keep_steps(a.H, shift);
  int m = a.sel_count[b];
  m = m < 0 ? 0 : (m > a.n_keep ? a.n_keep : m);
  const int32_t* sidx = a.sel_idx + (long)b * a.n_keep;
  const float* nb = a.noise + (long)b * RB * a.Kp;
  const float* Ub = a.U + (long)b * RB;
  float* vb = a.v + (long)b * RB * a.pitch;
  const int t0 = r0 - (int)((unsigned)r0 / (unsigned)a.H) * a.H;  // step of row r0 (one division per wave)

  const int j = lane + 64 * stride;
  if (j < a.pitch) {
    const int id = j < m ? sidx[j] : -1;
    const bool ok = (unsigned)id < (unsigned)a.K;
    float e[T], Ur[T];
    bool live[T];
    int t = t0;
#pragma unroll
    for (int i = 0; i < T; ++i) {
      const int r = r0 + i;
      live[i] = ok && r < RB && t < steps;  // (t < steps: row r + sh is a row of the same actuator)
      const int rs = r + sh < RB ? r + sh : RB - 1;
      e[i] = live[i] ? nb[(long)rs * a.Kp + id] : 0.0f;
      Ur[i] = Ub[rs];
      t = t + 1 == a.H ? 0 : t + 1;
    }
#pragma unroll
    for (int i = 0; i < T; ++i) {
      const int r = r0 + i;
      if (r < RB) vb[(long)r * a.pitch + j] = live[i] ? keep_store_v(Ur[i], e[i], a.clamp) : 0.0f;
    }
  }
  if (tile == 0 && stride == 0) {  // (wave-uniform) the set's header
    for (int j = lane; j < a.n_keep; j += 64) {
      const int id = j < m ? sidx[j] : -1;
      const bool ok = (unsigned)id < (unsigned)a.K;
      a.kcost[(long)b * a.n_keep + j] = ok ? a.costs[(long)b * a.Kp + id] : INFINITY;
      a.idx[(long)b * a.n_keep + j] = ok ? id : -1;
    }
    if (lane == 0) {
      a.count[b] = m;
      a.steps[b] = steps;
    }
  }
}

typedef float kf4 __attribute__((ext_vector_type(4)));

// The injection.  count[b] and steps[b] are read from device memory (wave-uniform), so a captured graph's first solve
// injects whatever set is stored when it replays; an empty set (either 0) exits before any other access.  Only columns
// j < count of rows t < steps are stored.  Lanes own 16-B quads of columns, q = lane + 64 i: a quad wholly below count is
// one 16-B load of v and one 16-B store (v's pitch and the noise rows are 16-B aligned); the ragged quad at the end
// stores its elements below count one by one.  Never a read-modify-write of a neighbouring column, so columns >= count
// in the same quad, the pads and the rows beyond steps come out bit for bit.
template <int T>
__global__ __launch_bounds__(256) void keep_inject_kernel(KeepArgs a, int tpb, int nwave) {
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (int)blockIdx.x * 4;
  if (w >= nwave) return;  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const int b = (int)((unsigned)w / (unsigned)tpb), tile = w - b * tpb;
  int cnt = a.count[b], st = a.steps[b];
  cnt = cnt > a.n_keep ? a.n_keep : cnt;  // (n_keep <= K <= Kp: column j < cnt is inside the row, and inside v's pitch)
  st = st > a.H ? a.H : st;
  if (cnt <= 0 || st <= 0) return;  // (wave-uniform) nothing stored
  const int RB = a.nu * a.H, r0 = tile * T;
  float* nb = a.noise + (long)b * RB * a.Kp;
  const float* Ub = a.U + (long)b * RB;
  const float* vb = a.v + (long)b * RB * a.pitch;
  const int t0 = r0 - (int)((unsigned)r0 / (unsigned)a.H) * a.H;

  for (int q = lane; 4 * q < cnt; q += 64) {
    const int j0 = 4 * q;  // (j0 + 3 < pitch: the quad lies inside v's row)
    kf4 x[T];
    float Ur[T];
    bool live[T];
    int t = t0;
#pragma unroll
    for (int i = 0; i < T; ++i) {
      const int r = r0 + i;
      live[i] = r < RB && t < st;
      const int rc = r < RB ? r : RB - 1;
      x[i] = live[i] ? *reinterpret_cast<const kf4*>(vb + (long)rc * a.pitch + j0) : kf4{0.0f, 0.0f, 0.0f, 0.0f};
      Ur[i] = Ub[rc];
      t = t + 1 == a.H ? 0 : t + 1;
    }
#pragma unroll
    for (int i = 0; i < T; ++i) {
      if (!live[i]) continue;
      float* p = nb + (long)(r0 + i) * a.Kp + j0;
      const kf4 o{keep_inject_eps(x[i].x, Ur[i]), keep_inject_eps(x[i].y, Ur[i]), keep_inject_eps(x[i].z, Ur[i]),
                  keep_inject_eps(x[i].w, Ur[i])};
      if (j0 + 3 < cnt) {
        *reinterpret_cast<kf4*>(p) = o;
      } else {  // the ragged end: elements below count alone
        p[0] = o.x;
        if (j0 + 1 < cnt) p[1] = o.y;
        if (j0 + 2 < cnt) p[2] = o.z;
      }
    }
  }
}

// MPPI_KEEP_ROWS=1|2|4|8 (read per launch; a test knob): force the rows a wave takes
static int keep_rows_knob() {
  const char* e = std::getenv("MPPI_KEEP_ROWS");
  const int v = e ? std::atoi(e) : 0;
  return (v == 1 || v == 2 || v == 4 || v == 8) ? v : 0;
}

static bool keep_args_ok(const KeepArgs& a) {
  const long rows = (long)a.B * a.nu * a.H;
  return a.B >= 1 && a.nu >= 1 && a.H >= 1 && a.K >= 1 && a.Kp >= a.K && a.n_keep >= 1 && a.n_keep <= a.K &&
         a.pitch >= a.n_keep && rows < (1L << 30);  // (rows and waves are 32-bit indices in the kernels)
}

// rows per wave: 8 while that leaves every CU at least 8 waves (`per_row` waves share a row tile), else fewer
static int keep_rows(const KeepArgs& a, int per_row = 1) {
  int T = keep_rows_knob();
  if (T) return T;
  const long want = 8L * current_device_cus(), rows = (long)a.B * a.nu * a.H;
  for (T = 8; T > 1 && rows / T * per_row < want; T >>= 1) {
  }
  return T;
}

hipError_t launch_keep_gather(const KeepArgs& a, int shift, hipStream_t stream) {
  if (!keep_args_ok(a) || (a.pitch & 3)) return hipErrorInvalidValue;
  const int ns = (a.pitch + 63) / 64;  // 64-column strides of the set: one wave each
  const int T = keep_rows(a, ns), RB = a.nu * a.H;
  const int tpb = (RB + T - 1) / T;
  const long lwave = (long)a.B * tpb * ns;
  if (lwave >= (1L << 30)) return hipErrorInvalidValue;
  const int nwave = (int)lwave;
  const dim3 grid((unsigned)((nwave + 3) / 4));
  auto kern = T == 8 ? keep_gather_kernel<8> : T == 4 ? keep_gather_kernel<4> : T == 2 ? keep_gather_kernel<2>
                                                                                       : keep_gather_kernel<1>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, a, shift, tpb, ns, nwave);
  return hipGetLastError();
}

hipError_t launch_keep_inject(const KeepArgs& a, hipStream_t stream) {
  if (!keep_args_ok(a)) return hipErrorInvalidValue;
  const int T = keep_rows(a), RB = a.nu * a.H;
  const int tpb = (RB + T - 1) / T, nwave = a.B * tpb;
  const dim3 grid((unsigned)((nwave + 3) / 4));
  auto kern = T == 8 ? keep_inject_kernel<8> : T == 4 ? keep_inject_kernel<4> : T == 2 ? keep_inject_kernel<2>
                                                                                       : keep_inject_kernel<1>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, a, tpb, nwave);
  return hipGetLastError();
}

}  // namespace mppi
