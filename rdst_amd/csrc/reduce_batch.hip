// See reduce_batch.h.
#include "reduce_batch.h"
#include <atomic>
#include <mutex>
#include <vector>

namespace rbatch {
namespace {

constexpr int MAXJ = 16;   // jobs per launch: a DenseSTLayer's backward (2 Swin blocks + its tail Linear) queues 11 sums and 5 finishes
struct SumBatch { SumJob j[MAXJ]; int first[MAXJ + 1]; int n; };   // first[k] = first block of job k
struct FinBatch { FinJob j[MAXJ]; int first[MAXJ + 1]; int n; };

thread_local bool g_active = false;
thread_local std::vector<SumJob> g_sums;
thread_local std::vector<FinJob> g_fins;

// one summed element -> its destination(s)
__device__ __forceinline__ void emit(const SumJob& J, int n, int c, int i, float a) {
  if (J.map == MAP_COPY) {
    J.out[J.g4 ? n * J.b2 + c : i] = a;
  } else if (J.map == MAP_LINEAR) {
    const int K = J.a, Kx = J.b;
    if (!J.g4) { n = i / Kx; c = i - n * Kx; }
    if (c < K) { if (J.out) J.out[(int64_t)n * K + c] = a * J.s; }
    else if (c == K && J.out2) J.out2[n] = a * J.s;
  } else if (J.map == MAP_MLP) {
    const int C = J.a, hid = J.b, n1 = hid * (C + 1);
    if (i < n1) J.out[i] = a;
    else {
      const int i2 = i - n1, jj = i2 / C, cc = i2 - jj * C;
      if (jj < hid) J.out2[(int64_t)cc * hid + jj] = a;
      else J.out3[cc] = a;
    }
  } else if (J.map == MAP_T) {
    const int rows = J.a;   // n = j, c = channel
    if (n < rows) J.out[(int64_t)c * rows + n] = a;
    else if (n == rows) J.out2[c] = a;
  } else {
    const int heads = J.a, T = J.b, hh = i / T, t = i - hh * T;
    J.out[t * heads + hh] = a;
  }
}

// sum of the slabs in fixed order: 32 outputs (fp32) or 32 groups of 4 (G4) per block, 8 slab groups x 8 loads in flight,
// two fixed-order levels
__global__ void __launch_bounds__(256) batched_sum_kernel(const SumBatch bt) {
  __shared__ float part[4][8][33];
  int k = 0;
#pragma unroll
  for (int q = 1; q < MAXJ; ++q) k += (q < bt.n && (int)blockIdx.x >= bt.first[q]) ? 1 : 0;
  const SumJob& J = bt.j[k];
  const int o = threadIdx.x & 31, sg = threadIdx.x >> 5;
  const int i = ((int)blockIdx.x - bt.first[k]) * 32 + o;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (i < J.tot) {
    if (J.g4) {
      const uint2* sl = reinterpret_cast<const uint2*>(J.slab);
      for (int w0 = sg; w0 < J.nwg; w0 += 8 * 8) {
        uint2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (w0 + 8 * u < J.nwg) ? sl[(int64_t)(w0 + 8 * u) * J.stride + i] : make_uint2(0u, 0u);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          a0 += __uint_as_float(v[u].x << 16); a1 += __uint_as_float(v[u].x & 0xffff0000u);
          a2 += __uint_as_float(v[u].y << 16); a3 += __uint_as_float(v[u].y & 0xffff0000u);
        }
      }
    } else {
      for (int w0 = sg; w0 < J.nwg; w0 += 8 * 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (w0 + 8 * u < J.nwg) ? J.slab[(int64_t)(w0 + 8 * u) * J.stride + i] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) a0 += v[u];
      }
    }
  }
  part[0][sg][o] = a0; part[1][sg][o] = a1; part[2][sg][o] = a2; part[3][sg][o] = a3;
  __syncthreads();
  if (sg != 0 || i >= J.tot) return;
  float r[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int q = 0; q < 8; ++q) r[e] += part[e][q][o];
  if (J.g4) {
    const int W = J.b2, ng = i / W, c = i - ng * W;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * ng + e < J.a2) emit(J, 4 * ng + e, c, 0, r[e]);
  } else {
    emit(J, 0, 0, i, r[0]);
  }
}

// LayerNorm finish, one block per 8 LayerNorm channels of one job (see linear_mfma.hip: wgrad_ln_finish_kernel)
__global__ void __launch_bounds__(1024) batched_ln_finish_kernel(const FinBatch bt) {
  __shared__ float pg[128][9], pb[128][9], qg[8][9], qb[8][9];
  int kj = 0;
#pragma unroll
  for (int q = 1; q < MAXJ; ++q) kj += (q < bt.n && (int)blockIdx.x >= bt.first[q]) ? 1 : 0;
  const FinJob& J = bt.j[kj];
  const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
  const int blk = (int)blockIdx.x - bt.first[kj];
  const int k = blk * 8 + tx;
  const int N = J.N, K = J.K, Kx = J.Kx;
  const float s = J.s;
  const float gk = k < K ? J.gamma[k] : 0.f, bk = k < K ? J.beta[k] : 0.f;
  float ag = 0.f, ab = 0.f;
#pragma unroll 3
  for (int n = ty; n < N; n += 128) {
    const float db = J.G[(int64_t)n * Kx + K];
    if (k < K) {
      const float g = J.G[(int64_t)n * Kx + k], w = J.Wt[(int64_t)n * K + k];
      if (J.dW) J.dW[(int64_t)n * K + k] = s * fmaf(gk, g, bk * db);
      ag = fmaf(w, g, ag);
      ab = fmaf(w, db, ab);
    }
    if (blk == 0 && tx == 0 && J.dbias) J.dbias[n] = s * db;
  }
  pg[ty][tx] = ag;
  pb[ty][tx] = ab;
  __syncthreads();
  if (ty < 8) {   // two fixed-order levels: 8 partial sums of 16 rows, then their sum
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) { a += pg[ty * 16 + j][tx]; b += pb[ty * 16 + j][tx]; }
    qg[ty][tx] = a;
    qb[ty][tx] = b;
  }
  __syncthreads();
  if (ty == 0 && k < K) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { a += qg[j][tx]; b += qb[j][tx]; }
    if (J.dgamma) J.dgamma[k] = s * a;
    if (J.dbeta) J.dbeta[k] = s * b;
  }
}

int launch_sums(const SumJob* jobs, int n, hipStream_t st) {
  for (int base = 0; base < n; base += MAXJ) {
    SumBatch bt{};
    bt.n = n - base < MAXJ ? n - base : MAXJ;
    int blocks = 0;
    for (int q = 0; q < bt.n; ++q) {
      bt.j[q] = jobs[base + q];
      bt.first[q] = blocks;
      blocks += (bt.j[q].tot + 31) / 32;
    }
    bt.first[bt.n] = blocks;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(batched_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, st, bt);
    if (int rc = rdst_launch_status("batched_sum")) return rc;
  }
  return 0;
}
int launch_fins(const FinJob* jobs, int n, hipStream_t st) {
  for (int base = 0; base < n; base += MAXJ) {
    FinBatch bt{};
    bt.n = n - base < MAXJ ? n - base : MAXJ;
    int blocks = 0;
    for (int q = 0; q < bt.n; ++q) {
      bt.j[q] = jobs[base + q];
      bt.first[q] = blocks;
      blocks += (bt.j[q].K + 7) / 8;
    }
    bt.first[bt.n] = blocks;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(batched_ln_finish_kernel, dim3((unsigned)blocks), dim3(1024), 0, st, bt);
    if (int rc = rdst_launch_status("batched_ln_finish")) return rc;
  }
  return 0;
}

}  // namespace

int sum(const SumJob& j, hipStream_t st) {
  if (g_active) { g_sums.push_back(j); return 0; }
  return launch_sums(&j, 1, st);
}
int finish(const FinJob& j, hipStream_t st) {
  if (g_active) { g_fins.push_back(j); return 0; }
  return launch_fins(&j, 1, st);
}

}  // namespace rbatch

// ------------------------------------------------------------------------------------------------
// The side branch (reduce_batch.h): one non-blocking stream per device on which rdst_reduce_batch_end() runs its two
// launches while the caller's stream goes on with the backward chain.  Ordering is by events alone.
// ------------------------------------------------------------------------------------------------
namespace rside {

constexpr int MAXDEV = 16;
constexpr int RING = 4;   // a generation takes two events (fork, close); a wait holds the record it was issued on, so two generations suffice
constexpr unsigned long long NO_CAPTURE = 0;

struct Dev {
  hipStream_t side = nullptr;
  hipEvent_t ev[RING] = {};
  bool ready = false;
  int next = 0;                       // ring slot of the next generation's fork event (its close event is next + 1)
  int pending = -1;                   // ring slot of the close event nobody waits for yet; -1: no generation pending
  unsigned long long pending_cap = NO_CAPTURE;   // id of the stream capture that event was recorded in (NO_CAPTURE: eagerly)
};

std::atomic<int> g_enabled{0};       // process-wide: set on the Python thread, read on autograd's device thread
std::mutex g_mu;                     // guards g_dev
Dev g_dev[MAXDEV];

int hip_fail(hipError_t e, const char* what) { return rdst_fail(-(int)e, "%s: %s", what, hipGetErrorString(e)); }

// the device `st` runs on, and the id of the capture it is part of (NO_CAPTURE outside one)
int where(hipStream_t st, int& dev, unsigned long long& cap) {
  hipError_t e = st ? hipStreamGetDevice(st, &dev) : hipGetDevice(&dev);
  if (e != hipSuccess) return hip_fail(e, "rdst_side: device of the stream");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  e = hipStreamGetCaptureInfo(st, &cs, &id);
  if (e != hipSuccess) return hip_fail(e, "rdst_side: hipStreamGetCaptureInfo");
  if (cs == hipStreamCaptureStatusInvalidated) return rdst_fail(RDST_EINVAL, "rdst_side: the stream's capture is invalidated");
  // (ids start at 1; the + 1 keeps NO_CAPTURE distinct whatever the runtime hands out)
  cap = cs == hipStreamCaptureStatusActive ? id + 1 : NO_CAPTURE;
  return 0;
}

int create(Dev& d, int dev) {
  int cur = -1;
  hipError_t e = hipGetDevice(&cur);
  if (e == hipSuccess && cur != dev) e = hipSetDevice(dev);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&d.side, hipStreamNonBlocking);
  for (int k = 0; k < RING && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&d.ev[k], hipEventDisableTiming);
  if (cur >= 0 && cur != dev) (void)hipSetDevice(cur);
  if (e != hipSuccess) {
    for (int k = 0; k < RING; ++k)
      if (d.ev[k]) { (void)hipEventDestroy(d.ev[k]); d.ev[k] = nullptr; }
    if (d.side) { (void)hipStreamDestroy(d.side); d.side = nullptr; }
    return hip_fail(e, "rdst_side: creating the side stream");
  }
  d.ready = true;
  d.next = 0;
  d.pending = -1;
  return 0;
}

// `st` waits for the pending generation, if it can: a generation recorded in a capture that is over (it failed, or it
// was left without a join and so could not be instantiated) is forgotten; an eager one cannot be waited for from inside
// a capture (that dependency would not be part of the graph): the caller has to join first.
int wait_pending(Dev& d, hipStream_t st, unsigned long long cap, const char* who) {
  if (d.pending < 0) return 0;
  if (d.pending_cap == cap) {
    hipError_t e = hipStreamWaitEvent(st, d.ev[d.pending], 0);
    if (e != hipSuccess) return hip_fail(e, who);
  } else if (d.pending_cap == NO_CAPTURE) {
    return rdst_fail(RDST_EINVAL, "%s: side work issued before this stream capture began is still pending (rdst_side_join first)", who);
  }
  d.pending = -1;
  return 0;
}

// steps (a) and (b); a single launch site (fork_begin: `reductions` false) takes (b) alone.  d stays null where the serial
// path has to be taken: nothing created yet and `st` is capturing, or a device index beyond the table.
int open_generation(hipStream_t st, Dev*& d, unsigned long long& cap, bool reductions = true) {
  int dev = 0;
  if (int rc = where(st, dev, cap)) return rc;
  if (dev < 0 || dev >= MAXDEV) return 0;
  Dev& D = g_dev[dev];
  if (!D.ready) {
    if (cap != NO_CAPTURE) return 0;   // never create a stream or an event while capturing
    if (int rc = create(D, dev)) return rc;
  }
  if (reductions) {
    if (int rc = wait_pending(D, st, cap, "rdst_reduce_batch_end")) return rc;
  } else if (D.pending >= 0 && D.pending_cap != cap) {
    // a single launch site does not wait for the generation before it (its own closing event will stand for both: the side
    // stream runs in order) - but that generation must belong to the same capture, or to none, as `st`
    if (D.pending_cap == NO_CAPTURE) return rdst_fail(RDST_EINVAL, "rdst_side: side work issued before this stream capture began is still pending");
    D.pending = -1;
  }
  hipError_t e = hipEventRecord(D.ev[D.next], st);
  if (e == hipSuccess) e = hipStreamWaitEvent(D.side, D.ev[D.next], 0);
  if (e != hipSuccess) return hip_fail(e, "rdst_reduce_batch_end: forking the side stream");
  d = &D;
  return 0;
}

// step (a) alone
int wait_only(hipStream_t st) {
  int dev = 0;
  unsigned long long cap = 0;
  if (int rc = where(st, dev, cap)) return rc;
  if (dev < 0 || dev >= MAXDEV || !g_dev[dev].ready) return 0;
  return wait_pending(g_dev[dev], st, cap, "rdst_reduce_batch_end");
}

// step (d)
int close_generation(Dev& d, unsigned long long cap) {
  const int slot = d.next + 1;
  hipError_t e = hipEventRecord(d.ev[slot], d.side);
  if (e != hipSuccess) return hip_fail(e, "rdst_reduce_batch_end: closing the side generation");
  d.pending = slot;
  d.pending_cap = cap;
  d.next = (d.next + 2) % RING;
  return 0;
}

// Forget every pending generation.  One that was issued eagerly may still be running and nothing will wait for it any
// more, so the host waits here (an error path); one recorded in a capture never ran.  Without a device nothing was ever
// created and no HIP call is made.
int forget_all(const char* who) {
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = 0;
  for (Dev& d : g_dev) {
    if (!d.ready || d.pending < 0) continue;
    if (d.pending_cap == NO_CAPTURE) {
      hipError_t e = hipStreamSynchronize(d.side);
      if (e != hipSuccess && !rc) rc = hip_fail(e, who);
    }
    d.pending = -1;
  }
  return rc;
}

int fork_begin(hipStream_t st, Fork& f) {
  f.run = st;
  f.dev = nullptr;
  if (!(g_enabled.load(std::memory_order_relaxed) & SIDE_CONV)) return 0;
  std::lock_guard<std::mutex> lk(g_mu);
  Dev* d = nullptr;
  if (int rc = open_generation(st, d, f.cap, false)) return rc;
  if (d) { f.dev = d; f.run = d->side; }
  return 0;
}
int fork_end(Fork& f) {
  if (!f.dev) return 0;
  std::lock_guard<std::mutex> lk(g_mu);
  Dev* d = static_cast<Dev*>(f.dev);
  f.dev = nullptr;
  return close_generation(*d, f.cap);
}

}  // namespace rside

extern "C" int rdst_reduce_batch_begin(void) {
  if (rbatch::g_active) return rdst_fail(RDST_EINVAL, "rdst_reduce_batch_begin: a batch is already open on this thread");
  rbatch::g_active = true;
  rbatch::g_sums.clear();
  rbatch::g_fins.clear();
  return 0;
}

extern "C" int rdst_reduce_batch_end(void* stream) {
  if (!rbatch::g_active) return rdst_fail(RDST_EINVAL, "rdst_reduce_batch_end: no open batch");
  rbatch::g_active = false;
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  if (const int bits = rside::g_enabled.load(std::memory_order_relaxed)) {
    // the side branch: (a) `st` behind the previous generation, (b) the side stream behind `st`, (c) the same two launches
    // there, (d) the generation's closing event.  A generation that was opened is always closed, so a join finds its end.
    // With the conv stage alone, (a) is all that happens: the launches stay on `st`, behind the weight gradients issued so far.
    std::lock_guard<std::mutex> lk(rside::g_mu);
    rside::Dev* d = nullptr;
    unsigned long long cap = 0;
    rc = (bits & rside::SIDE_REDUCE) ? rside::open_generation(st, d, cap) : rside::wait_only(st);
    hipStream_t run = d ? d->side : st;
    if (!rc) rc = rbatch::launch_sums(rbatch::g_sums.data(), (int)rbatch::g_sums.size(), run);
    if (!rc) rc = rbatch::launch_fins(rbatch::g_fins.data(), (int)rbatch::g_fins.size(), run);
    if (d) {
      const int rc2 = rside::close_generation(*d, cap);
      if (!rc) rc = rc2;
    }
  } else {
    rc = rbatch::launch_sums(rbatch::g_sums.data(), (int)rbatch::g_sums.size(), st);
    if (!rc) rc = rbatch::launch_fins(rbatch::g_fins.data(), (int)rbatch::g_fins.size(), st);
  }
  rbatch::g_sums.clear();
  rbatch::g_fins.clear();
  return rc;
}

extern "C" int rdst_reduce_batch_abort(void) {
  // drop whatever is queued WITHOUT running it (the workspaces and outputs of a failed backward may be gone)
  rbatch::g_active = false;
  rbatch::g_sums.clear();
  rbatch::g_fins.clear();
  return rside::forget_all("rdst_reduce_batch_abort");   // (the side work already issued wrote into the same dead pass)
}

extern "C" int rdst_side_enable(int on) { return rside::g_enabled.exchange(on & (rside::SIDE_REDUCE | rside::SIDE_CONV)); }

extern "C" int rdst_side_join(void* stream) {
  std::lock_guard<std::mutex> lk(rside::g_mu);
  hipStream_t st = (hipStream_t)stream;
  int dev = 0;
  unsigned long long cap = 0;
  if (int rc = rside::where(st, dev, cap)) return rc;
  if (dev < 0 || dev >= rside::MAXDEV || !rside::g_dev[dev].ready) return 0;
  return rside::wait_pending(rside::g_dev[dev], st, cap, "rdst_side_join");
}

extern "C" int rdst_side_reset(void) { return rside::forget_all("rdst_side_reset"); }
