// Launch interface of the batch verify kernels (ec_verify.hip): classify
// fragments resident in HBM by their headers and payload CRC-32.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ecamd {

// A payload's full 1 KiB chunks are cut into runs of this many; one work
// item of the chunk kernel is one run (a wave takes four chunks of it).
constexpr uint32_t kVerifyRunChunks = 16;

// Fragment (o, i) at frags + o*stripe_stride + i*frag_stride, i < nfrag,
// checked when bit i of present[o] is set.  result[o] = {bad_header mask,
// bad_chksum mask} (frag_check.hpp for the header half; bad_chksum: the
// header's chksum_mismatch flag, or a CHKSUM_CRC32 payload whose stored
// chksum[0] is neither variant's CRC of the bs payload bytes).  Nothing is
// written to frags; bytes past 80 + bs of a slot are never read.
struct VerifyParams {
  const uint8_t* frags;
  uint64_t frag_stride, stripe_stride;
  uint64_t obj_len;
  uint32_t bs;
  uint32_t n_obj, nfrag;
  uint32_t wire_id;         // backend id the instance writes into headers
  const uint32_t* present;  // n_obj masks, device memory
  uint32_t* state;          // n_obj * nfrag: 1 while the payload CRC is still unmatched
  uint32_t* part;           // n_obj * nfrag * (bs / 1024) chunk partials
  uint32_t* result;         // n_obj x 2, device memory
  const void* lanes[2];     // CrcLaneTables (crc32.hpp): zlib, legacy
  const void* tables[2];    // CrcFinishTables for bs: zlib, legacy
};

// state / part sizes in u32 (one buffer: state first).
inline uint64_t verify_state_words(uint32_t n_obj, uint32_t nfrag) {
  return (static_cast<uint64_t>(n_obj) * nfrag + 3) & ~uint64_t(3);
}
inline uint64_t verify_part_words(uint32_t n_obj, uint32_t nfrag, uint32_t bs) {
  return static_cast<uint64_t>(n_obj) * nfrag * (bs / 1024);
}

// Zeroes result, then: headers; chunk CRCs and compare with the zlib tables
// over every fragment; the same with the legacy tables over the fragments
// the first pass left unmatched (decided on the device).  Asynchronous.
hipError_t launch_verify(const VerifyParams& p, hipStream_t stream);

}  // namespace ecamd
