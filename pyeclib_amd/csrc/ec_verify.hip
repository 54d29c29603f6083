// Batch verify: classify fragments resident in HBM (ecamd_verify_batch).
//
// The read side of the inline CRC-32.  Three kernels, all read-only over the
// fragments:
//   * verify_header_kernel -- one thread per fragment slot: the 80-byte
//     header into registers, frag_check.hpp's classification (shared with
//     the host), the bad_header / chksum_mismatch bits, and state[f] = 1 for
//     a sound CHKSUM_CRC32 fragment whose payload is to be checked.
//   * verify_chunks_kernel -- the payloads' full 1 KiB chunks, cut into runs
//     of kVerifyRunChunks so that one object still fills the device: a work
//     item is one run of one fragment, a wave takes four of its chunks (four
//     16-byte loads per lane, each chunk read from HBM once), each chunk's
//     raw CRC on the matrix cores (8 bit planes, crc_device.hpp mfma_plane),
//     the four lookups per lane, and one wave XOR for the four.  Blocks are
//     persistent (the 16 KiB second-stage table is copied to LDS once, and
//     only by a block that finds work).
//   * verify_fold_kernel -- one block per fragment: the chunk partials folded
//     to the payload's end as crc_finish_kernel does (runs per thread by
//     Z_1024, the lane tree, the waves), the bs mod 1024 tail read back as
//     one end-aligned chunk, the init term; the result compared with the
//     header's chksum[0].  A match clears state[f].
// The chunk and fold kernels run twice, with the zlib tables and then with
// the legacy ones; the second pass skips every fragment whose state the first
// cleared (a block-uniform test of device memory: no host round trip), and
// reports what is still unmatched.
#include <algorithm>
#include <cstddef>

#include "crc32.hpp"
#include "crc_device.hpp"
#include "ec_verify.hpp"
#include "frag_check.hpp"

namespace ecamd {
namespace {

using crcdev::lds32;
using crcdev::zmap;

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4u lds_v4u;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kHeaderBytes = 80;
constexpr uint32_t kWaveChunks = 4;  // one wave_xor4
static_assert(kVerifyRunChunks == kWaveChunks * (kThreads / 64), "a run is one block's chunks");

__device__ __forceinline__ const uint8_t* frag_at(const VerifyParams& p, uint64_t f, uint32_t* o,
                                                  uint32_t* i) {
  *o = static_cast<uint32_t>(f / p.nfrag);
  *i = static_cast<uint32_t>(f - static_cast<uint64_t>(*o) * p.nfrag);
  return p.frags + static_cast<uint64_t>(*o) * p.stripe_stride + static_cast<uint64_t>(*i) * p.frag_stride;
}

__global__ void __launch_bounds__(kThreads) verify_header_kernel(VerifyParams p) {
  const uint64_t f = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= static_cast<uint64_t>(p.n_obj) * p.nfrag) return;
  uint32_t o, i;
  const uint8_t* frag = frag_at(p, f, &o, &i);
  uint32_t st = 0;
  if (p.present[o] >> i & 1u) {
    const uint4* h = reinterpret_cast<const uint4*>(frag);  // slots are 16-byte aligned
    uint32_t w[fragcheck::kHeaderDwords];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const uint4 x = h[q];
      w[4 * q] = x.x;
      w[4 * q + 1] = x.y;
      w[4 * q + 2] = x.z;
      w[4 * q + 3] = x.w;
    }
    const int v = fragcheck::classify_header(w, p.wire_id, i, p.bs, p.obj_len);
    if (v == fragcheck::kBadHeader)
      atomicOr(&p.result[2 * static_cast<uint64_t>(o)], 1u << i);
    else if (v == fragcheck::kMismatchFlag)
      atomicOr(&p.result[2 * static_cast<uint64_t>(o) + 1], 1u << i);
    else if (fragcheck::hdr8(w, 20) == fragcheck::kChksumCrc32)
      st = 1;
  }
  p.state[f] = st;
}

// LDS: CrcLaneTables::mst at byte 0.
constexpr uint32_t kChunkLds = sizeof(CrcLaneTables::mst);
static_assert(kChunkLds % 16 == 0, "copied in 16-B pieces");

// Block b takes the items [b * per, (b + 1) * per) -- consecutive runs of
// one fragment, then of the next -- so it reads a fragment's state once and
// steps over a cleared fragment's runs in one go (the second pass of a clean
// batch costs a few loads per block).
// Four waves per SIMD asked for: with at most 128 registers the row sums stay
// in VGPRs (no AGPR read-back before the lookups), and one chunk's eight
// planes are issued as one chain before the next chunk's (a single
// accumulator chain keeps the matrix pipe as busy as four, at a quarter of
// the registers) -- 8 % faster on the headline batch than the compiler's own
// choice of four interleaved AGPR accumulators.
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 8))) verify_chunks_kernel(VerifyParams p, int variant) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lane4 = 4 * lane;
  const uint32_t nfull = p.bs >> 10;
  const uint32_t runs = (nfull + kVerifyRunChunks - 1) / kVerifyRunChunks;
  const uint64_t items = static_cast<uint64_t>(p.n_obj) * p.nfrag * runs;
  const uint64_t per = (items + gridDim.x - 1) / gridDim.x;
  const uint64_t begin = blockIdx.x * per, end = begin + per < items ? begin + per : items;
  if (begin >= end) return;
  const void* lanes = p.lanes[variant];
  crcdev::mfma_v4i mb[8];
  bool loaded = false;
  uint64_t f = begin / runs;
  uint32_t run = static_cast<uint32_t>(begin - f * runs);
  for (uint64_t it = begin; it < end; ++f, run = 0) {
    // fragment f's runs [run, rend)
    const uint32_t rend = end - it < runs - run ? run + static_cast<uint32_t>(end - it) : runs;
    it += rend - run;
    if (p.state[f] == 0) continue;  // the same for the whole block
    if (!loaded) {
      auto* dst = reinterpret_cast<lds_v4u*>(static_cast<uintptr_t>(0));
      const v4u* src = reinterpret_cast<const v4u*>(static_cast<const char*>(lanes) + offsetof(CrcLaneTables, mst));
      for (uint32_t j = threadIdx.x; j < kChunkLds / 16; j += kThreads) dst[j] = src[j];
      crcdev::mfma_load_b(lanes, lane, mb);
      __syncthreads();
      loaded = true;
    }
    uint32_t o, i;
    const uint8_t* pay = frag_at(p, f, &o, &i) + kHeaderBytes + 16 * lane;
    uint32_t* part = p.part + f * nfull;
    // this wave's four chunks of run r (those past the last full chunk: zeros)
    auto load = [&](uint32_t r, uint4 (&x)[kWaveChunks]) {
      const uint32_t c0 = r * kVerifyRunChunks + wave * kWaveChunks;
#pragma unroll
      for (uint32_t q = 0; q < kWaveChunks; ++q)
        x[q] = c0 + q < nfull ? *reinterpret_cast<const uint4*>(pay + static_cast<uint64_t>(c0 + q) * 1024)
                              : make_uint4(0, 0, 0, 0);
    };
    uint4 x[kWaveChunks];
    load(run, x);
    for (uint32_t r = run; r < rend; ++r) {
      const uint32_t c0 = r * kVerifyRunChunks + wave * kWaveChunks;
      if (c0 < nfull) {  // the fragment's last run may be short
        uint32_t fin[kWaveChunks];
#pragma unroll
        for (uint32_t q = 0; q < kWaveChunks; ++q) {
          crcdev::mfma_v16i acc = {};
#pragma unroll
          for (int d = 0; d < 8; ++d) acc = crcdev::mfma_plane(x[q], d, mb[d], d == 0 ? crcdev::mfma_v16i{} : acc);
          fin[q] = crcdev::mfma_lanes(acc, 0, lane4);
          __builtin_amdgcn_sched_barrier(0);
        }
        const uint32_t t = crcdev::wave_xor4(fin[0], fin[1], fin[2], fin[3], lane);
        if (lane < kWaveChunks && c0 + lane < nfull) part[c0 + lane] = t;
      }
      if (r + 1 < rend) load(r + 1, x);
    }
  }
}

// LDS of the fold: the raw16 table (CrcLaneTables::raw16) at 0,
// CrcFinishTables after it, 8 wave partials (as ec_crc.hip).
constexpr uint32_t kFin = sizeof(CrcLaneTables::raw16);
constexpr uint32_t kPow = kFin + offsetof(CrcFinishTables, pow);
constexpr uint32_t kZr = kFin + offsetof(CrcFinishTables, zr);
constexpr uint32_t kZ16 = kFin + offsetof(CrcFinishTables, z16);
constexpr uint32_t kInit = kFin + offsetof(CrcFinishTables, init_term);
constexpr uint32_t kRed = kFin + sizeof(CrcFinishTables);
constexpr uint32_t kFoldLds = kRed + 32;
static_assert(offsetof(CrcLaneTables, raw16) == 0 && kFin % 16 == 0, "raw16 first");

// 16 payload bytes at [start, start + 16), those outside [lo, hi) as zero.
__device__ __forceinline__ uint4 window16(const uint8_t* pay, int64_t start, int64_t lo, int64_t hi) {
  if (start >= lo && start + 16 <= hi) {
    uint4 x;
    __builtin_memcpy(&x, pay + start, 16);  // unaligned when bs is not a multiple of 16
    return x;
  }
  uint32_t w[4] = {0, 0, 0, 0};
  if (start + 16 > lo && start < hi)
    for (int b = 0; b < 16; ++b) {
      const int64_t at = start + b;
      if (at >= lo && at < hi) w[b >> 2] |= static_cast<uint32_t>(pay[at]) << (8 * (b & 3));
    }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// ec_crc.hip lane_tree: 64 consecutive pieces, piece l in lane l, joined by
// tab_k = Z_{unit 2^k} at LDS byte tab + 512 k; the result is lane 63's.
__device__ __forceinline__ uint32_t lane_tree(uint32_t v, uint32_t tab) {
#pragma unroll
  for (int k = 0; k < 6; ++k) v = zmap(__shfl_up(v, 1u << k, 64), tab + 512u * k) ^ v;
  return __shfl(v, 63, 64);
}

__global__ void __launch_bounds__(kThreads) verify_fold_kernel(VerifyParams p, int variant, int last) {
  auto* red = reinterpret_cast<__attribute__((address_space(3))) uint32_t*>(static_cast<uintptr_t>(kRed));
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t n = p.bs >> 10;  // every full chunk has a partial
  // runs of L = 2^lg chunks per thread, 256 L >= n; the 256 L - n virtual
  // chunks in front are zeros (a zero prefix leaves a raw CRC unchanged)
  uint32_t lg = 0;
  while ((kThreads << lg) < n) ++lg;
  const uint32_t L = 1u << lg;
  const int64_t lead = static_cast<int64_t>(kThreads << lg) - n;
  const int64_t e0 = static_cast<int64_t>(n) * 1024, bs = p.bs;
  const uint64_t total = static_cast<uint64_t>(p.n_obj) * p.nfrag;
  bool loaded = false;
  for (uint64_t f = blockIdx.x; f < total; f += gridDim.x) {
    if (p.state[f] == 0) continue;  // the same for the whole block
    if (!loaded) {
      auto* dst = reinterpret_cast<lds_v4u*>(static_cast<uintptr_t>(0));
      const v4u* raw16 = reinterpret_cast<const v4u*>(p.lanes[variant]);
      for (uint32_t j = threadIdx.x; j < kFin / 16; j += kThreads) dst[j] = raw16[j];
      const v4u* fin = reinterpret_cast<const v4u*>(p.tables[variant]);
      for (uint32_t j = threadIdx.x; j < sizeof(CrcFinishTables) / 16; j += kThreads) dst[kFin / 16 + j] = fin[j];
      __syncthreads();
      loaded = true;
    }
    uint32_t o, i;
    const uint8_t* frag = frag_at(p, f, &o, &i);
    const uint8_t* pay = frag + kHeaderBytes;
    const uint32_t* part = p.part + f * n;
    // this thread's run, then the lane tree (Z_{1024 L 2^k} = pow[lg + k])
    uint32_t acc = 0;
    for (uint32_t j = 0; j < L; ++j) {
      const int64_t c = static_cast<int64_t>(threadIdx.x) * L + j - lead;
      const uint32_t x = c >= 0 ? part[c] : 0u;
      acc = (j == 0 ? 0u : zmap(acc, kPow)) ^ x;
    }
    acc = lane_tree(acc, kPow + 512u * lg);
    // the tail [e0, bs) as one chunk ending at bs (wave 0)
    uint32_t edge = 0;
    if (wave == 0 && bs > e0)
      edge = lane_tree(crcdev::raw16(window16(pay, bs - 1024 + 16 * static_cast<int64_t>(lane), e0, bs), 0), kZ16);
    if (lane == 0) {
      red[wave] = acc;
      red[4 + wave] = edge;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      // the four waves' runs (64 L chunks each) joined by Z_{1024 64 L},
      // then shifted by bs mod 1024
      uint32_t a = red[0];
      for (int w = 1; w < 4; ++w) a = zmap(a, kPow + 512u * (lg + 6)) ^ red[w];
      const uint32_t crc = zmap(a, kZr) ^ red[4] ^ lds32(kInit);
      uint32_t stored = 0;
      for (int b = 0; b < 4; ++b) stored |= static_cast<uint32_t>(frag[21 + b]) << (8 * b);
      if (crc == stored)
        p.state[f] = 0;
      else if (last)
        atomicOr(&p.result[2 * static_cast<uint64_t>(o) + 1], 1u << i);
    }
    __syncthreads();  // red[] is reused by the next fragment
  }
}

}  // namespace

hipError_t launch_verify(const VerifyParams& p, hipStream_t stream) {
  const uint64_t total = static_cast<uint64_t>(p.n_obj) * p.nfrag;
  if (total == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(p.result, 0, static_cast<size_t>(p.n_obj) * 2 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess)
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  hipLaunchKernelGGL(verify_header_kernel, dim3(static_cast<uint32_t>((total + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, stream, p);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const uint32_t nfull = p.bs >> 10;
  const uint64_t items = total * ((nfull + kVerifyRunChunks - 1) / kVerifyRunChunks);
  // the chunk kernel's blocks split the items evenly: as many as are
  // resident at once, so they all end together
  static const int chunk_blocks = [] {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, verify_chunks_kernel, kThreads, kChunkLds) != hipSuccess || n < 1)
      n = 4;
    return n;
  }();
  const uint64_t chunk_grid = static_cast<uint64_t>(cus) * chunk_blocks;
  // eight of the fold's blocks fit a CU
  const uint64_t resident = static_cast<uint64_t>(cus) * 8;
  for (int v = 0; v < 2; ++v) {
    if (items != 0) {
      hipLaunchKernelGGL(verify_chunks_kernel, dim3(static_cast<uint32_t>(std::min(items, chunk_grid))),
                         dim3(kThreads), kChunkLds, stream, p, v);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(verify_fold_kernel, dim3(static_cast<uint32_t>(std::min(total, resident))),
                       dim3(kThreads), kFoldLds, stream, p, v, v);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace ecamd
