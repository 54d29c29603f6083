// Header classification of a stored fragment, shared by the batch verify
// kernel (ec_verify.hip) and the host (ecamd_classify_header): what
// liberasurecode checks before it trusts a fragment -- is_invalid_fragment_header
// and is_invalid_fragment (upstream erasurecode_helpers.c / erasurecode.c;
// header_invalid and fragment_invalid in ec_runtime.cpp) -- plus the batch
// layout's own assumptions (slot, payload size, object length).
//
// The header is taken as its 20 little-endian dwords so that the device side
// keeps it in registers: every index below is a constant once the loops are
// unrolled (a byte array indexed at run time would live in scratch).  The two
// metadata CRCs are bitwise -- no table, so no LDS and no host state.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ECAMD_HD __host__ __device__
#else
#define ECAMD_HD
#endif

namespace ecamd {
namespace fragcheck {

constexpr int kHeaderDwords = 20;            // 80 bytes
constexpr uint32_t kMagic = 0xb0c5ecc;       // LIBERASURECODE_FRAG_HEADER_MAGIC
constexpr uint32_t kMaxVersion = 0x010800;   // newest fragment format understood
constexpr uint32_t kNoMagicBelow = 0x010200; // older writers: no magic, no metadata checksum
constexpr int kMetaBytes = 59;               // fragment_metadata_t, covered by the checksum at 67
constexpr uint32_t kChksumNone = 1, kChksumCrc32 = 2, kChksumMd5 = 3;

enum Verdict : int { kOk = 0, kBadHeader = 1, kMismatchFlag = 2 };

// Byte / dword at a constant byte offset of the header.
ECAMD_HD inline uint32_t hdr8(const uint32_t (&w)[kHeaderDwords], int at) {
  return (w[at >> 2] >> (8 * (at & 3))) & 0xFFu;
}
ECAMD_HD inline uint32_t hdr32(const uint32_t (&w)[kHeaderDwords], int at) {
  const int d = at >> 2, s = 8 * (at & 3);
  return s == 0 ? w[d] : (w[d] >> s) | (w[d + 1] << (32 - s));
}

// One table entry of the reflected CRC-32, computed: T0[n].
ECAMD_HD inline uint32_t crc_t0(uint32_t n) {
  for (int b = 0; b < 8; ++b) n = (n >> 1) ^ (0xEDB88320u & (0u - (n & 1u)));
  return n;
}

// crc32(0, header, 59) in zlib's form and in liberasurecode's legacy one
// (signed accumulator: the right shift is arithmetic; crc32.hpp).
ECAMD_HD inline void meta_crcs(const uint32_t (&w)[kHeaderDwords], uint32_t* zlib, uint32_t* legacy) {
  uint32_t z = 0xFFFFFFFFu, l = 0xFFFFFFFFu;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int d = 0; d < (kMetaBytes + 3) / 4; ++d) {
    const uint32_t word = w[d];
    const int nb = kMetaBytes - 4 * d < 4 ? kMetaBytes - 4 * d : 4;
    for (int b = 0; b < nb; ++b) {
      const uint32_t byte = (word >> (8 * b)) & 0xFFu;
      z = crc_t0((z ^ byte) & 0xFFu) ^ (z >> 8);
      l = crc_t0((l ^ byte) & 0xFFu) ^ static_cast<uint32_t>(static_cast<int32_t>(l) >> 8);
    }
  }
  *zlib = ~z;
  *legacy = ~l;
}

// The fragment found in slot `slot` of an object of obj_len bytes whose
// payloads are `blocksize` bytes, on an instance that writes `wire_id` into
// its headers.  kMismatchFlag: the header is sound and carries
// chksum_mismatch = 1.
ECAMD_HD inline int classify_header(const uint32_t (&w)[kHeaderDwords], uint32_t wire_id, uint32_t slot,
                                    uint64_t blocksize, uint64_t obj_len) {
  const uint32_t ver = hdr32(w, 63), magic = hdr32(w, 59);
  if (ver == 0) return kBadHeader;
  if (ver >= kNoMagicBelow) {
    if (magic != kMagic) return kBadHeader;
    uint32_t z, l;
    meta_crcs(w, &z, &l);
    const uint32_t stored = hdr32(w, 67);
    if (stored != z && stored != l) return kBadHeader;
  }
  if (ver > kMaxVersion) return kBadHeader;
  if (magic != kMagic) return kBadHeader;
  if (hdr8(w, 54) != wire_id) return kBadHeader;
  const uint32_t ct = hdr8(w, 20);
  if (ct < kChksumNone || ct > kChksumMd5) return kBadHeader;
  const uint64_t orig = static_cast<uint64_t>(hdr32(w, 12)) | static_cast<uint64_t>(hdr32(w, 16)) << 32;
  if (hdr32(w, 0) != slot || hdr32(w, 4) != blocksize || orig != obj_len) return kBadHeader;
  if (hdr8(w, 53) == 1) return kMismatchFlag;
  return kOk;
}

}  // namespace fragcheck
}  // namespace ecamd
