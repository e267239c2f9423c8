// kvidx_common.h - shared table layout + hashing for the KV-block index.
//
// The block->pod index is an open-addressing hash table designed to live in
// MI355X HBM3E (288 GB/GPU) and be probed by wave-cooperative HIP kernels;
// the exact same layout is operated on by the CPU reference implementation
// (cpu_ops.cpp) so CPU<->GPU differential tests are bit-exact.
//
// Behavioral parity notes (reference: /root/reference, Go):
//  - chunk hash = FNV-64a(canonical CBOR [parent, chunk, null])
//    (pkg/kvcache/kvblock/token_processor.go:94-112)
//  - dual keys: engine map (engine hash -> request hash) feeds eviction and
//    parent-chain stitching (pkg/kvcache/kvblock/in_memory.go:159-167)
//  - per-key pod set with bounded capacity (default 10,
//    in_memory.go:32-35); approximate LRU via epoch stamps.
//
// Layout (structure-of-arrays, all torch tensors):
//   keys  : int64 [C]    chunk hash; 0 = never-used (free). A real hash of
//                        0 is remapped to 1 (KVIDX_REMAP).
//   meta  : int32 [C]    bit31 OCC, bit30 TOMB, bits 0..15 model_id
//   stamp : int32 [C]    last-touch epoch (approximate LRU)
//   pods  : int32 [C*P]  pod entries; 0 = empty,
//                        else (tier<<24) | (pod_id+1)  (pod_id < 2^24-1)
//   e_keys/e_meta/e_vals: the engine->request map (same C, e_vals holds the
//                        request hash)

#pragma once

#include <cstdint>

// Debug asserts (ROADMAP r1 #10): compile with KVIDX_DEBUG=1 in the
// environment (setup.py adds -DKVIDX_DEBUG_ASSERTS) to trap on
// violated kernel/table invariants - a hipMemcheck-style guard with
// zero cost in release builds.
#ifdef KVIDX_DEBUG_ASSERTS
#if defined(__HIP_DEVICE_COMPILE__)
#define KVIDX_ASSERT(c) \
  do {                  \
    if (!(c)) __builtin_trap(); \
  } while (0)
#else
#include <cassert>
#define KVIDX_ASSERT(c) assert(c)
#endif
#else
#define KVIDX_ASSERT(c) ((void)0)
#endif

#if defined(__HIPCC__)
#define KVIDX_HD __host__ __device__ __forceinline__
#else
#define KVIDX_HD inline
#endif

namespace kvidx {

static constexpr uint64_t FNV64_OFFSET = 0xCBF29CE484222325ull;
static constexpr uint64_t FNV64_PRIME = 0x100000001B3ull;

static constexpr uint32_t META_OCC = 0x80000000u;
static constexpr uint32_t META_TOMB = 0x40000000u;
static constexpr uint32_t META_MODEL_MASK = 0xFFFFu;

static constexpr int MAX_TIERS = 4;
static constexpr int PROBE_MAX = 128;

KVIDX_HD uint64_t remap_hash(uint64_t h) { return h == 0 ? 1ull : h; }

KVIDX_HD uint64_t kvidx_checked_slot(uint64_t i, uint64_t cap_mask) {
  KVIDX_ASSERT(i <= cap_mask);
  return i;
}

// (h ^ b) * FNV64_PRIME, with the product by 2^40 + 0x1B3 written out in
// 32-bit halves: on gfx950 that is a multiply, a shift-add and one
// multiply-add with the high half folded in as its addend, against four
// multiply-group instructions for the plain 64-bit product.
KVIDX_HD uint64_t fnv1a_64_byte(uint64_t h, uint8_t b) {
  static_assert(FNV64_PRIME == ((1ull << 40) | 0x1B3ull), "split below");
  const uint32_t lo = (uint32_t)h ^ (uint32_t)b;
  const uint32_t t = (uint32_t)(h >> 32) * 0x1B3u + (lo << 8);
  return (uint64_t)lo * 0x1B3u + ((uint64_t)t << 32);
}

// Canonical-CBOR unsigned integer append; returns new length.
KVIDX_HD int cbor_put_uint(uint8_t* buf, int len, uint64_t v, uint8_t major) {
  const uint8_t mt = major << 5;
  if (v < 24) {
    buf[len++] = mt | (uint8_t)v;
  } else if (v <= 0xFF) {
    buf[len++] = mt | 24;
    buf[len++] = (uint8_t)v;
  } else if (v <= 0xFFFF) {
    buf[len++] = mt | 25;
    buf[len++] = (uint8_t)(v >> 8);
    buf[len++] = (uint8_t)v;
  } else if (v <= 0xFFFFFFFFull) {
    buf[len++] = mt | 26;
    buf[len++] = (uint8_t)(v >> 24);
    buf[len++] = (uint8_t)(v >> 16);
    buf[len++] = (uint8_t)(v >> 8);
    buf[len++] = (uint8_t)v;
  } else {
    buf[len++] = mt | 27;
    for (int s = 56; s >= 0; s -= 8) buf[len++] = (uint8_t)(v >> s);
  }
  return len;
}

// Streaming canonical-CBOR unsigned integer fed straight into FNV-64a -
// no byte buffer, so GPU lanes keep everything in registers (no scratch).
KVIDX_HD uint64_t fnv_cbor_uint(uint64_t h, uint64_t v, uint8_t major) {
  const uint8_t mt = major << 5;
  if (v < 24) {
    h = fnv1a_64_byte(h, mt | (uint8_t)v);
  } else if (v <= 0xFF) {
    h = fnv1a_64_byte(h, mt | 24);
    h = fnv1a_64_byte(h, (uint8_t)v);
  } else if (v <= 0xFFFF) {
    h = fnv1a_64_byte(h, mt | 25);
    h = fnv1a_64_byte(h, (uint8_t)(v >> 8));
    h = fnv1a_64_byte(h, (uint8_t)v);
  } else if (v <= 0xFFFFFFFFull) {
    h = fnv1a_64_byte(h, mt | 26);
    for (int s = 24; s >= 0; s -= 8) h = fnv1a_64_byte(h, (uint8_t)(v >> s));
  } else {
    h = fnv1a_64_byte(h, mt | 27);
    for (int s = 56; s >= 0; s -= 8) h = fnv1a_64_byte(h, (uint8_t)(v >> s));
  }
  return h;
}

// Branchless (predicated) variants: identical output to fnv_cbor_uint but
// straight-line code, so lanes of a wave never diverge on the
// data-dependent encoding lengths.  One wave alone on a SIMD is
// issue-bound (about 5 cycles per vector instruction whatever it is), so
// what counts here is the number of instructions, not their latency:
//  - a u32 has 0, 1, 2 or 4 value bytes, never 3, so the two high bytes
//    share one predicate and run back to back under ONE 64-bit select;
//  - all three predicates and the header byte depend on v alone and are
//    computed ahead of the first step, which leaves the compiler free to
//    place each compare well before the select that reads it (a compare
//    directly in front of its select costs a hazard nop).
KVIDX_HD uint64_t fnv_cbor_u32_branchless(uint64_t h, uint32_t v,
                                          uint8_t major) {
  const uint8_t mt = major << 5;
  const bool p1 = v >= 24;      // at least one value byte
  const bool p2 = v > 0xFF;     // at least two
  const bool p4 = v > 0xFFFF;   // four
  const uint8_t info = p4 ? 26 : p2 ? 25 : p1 ? 24 : (uint8_t)v;
  h = fnv1a_64_byte(h, (uint8_t)(mt | info));
  const uint64_t h4 = fnv1a_64_byte(fnv1a_64_byte(h, (uint8_t)(v >> 24)),
                                    (uint8_t)(v >> 16));
  h = p4 ? h4 : h;
  const uint64_t h2 = fnv1a_64_byte(h, (uint8_t)(v >> 8));
  h = p2 ? h2 : h;
  const uint64_t h1 = fnv1a_64_byte(h, (uint8_t)v);
  h = p1 ? h1 : h;
  return h;
}

KVIDX_HD uint64_t fnv_cbor_u64_branchless(uint64_t h, uint64_t v,
                                          uint8_t major) {
  const uint8_t mt = major << 5;
  const int sel = (v >= 24) + (v > 0xFF) + (v > 0xFFFF) +
                  (v > 0xFFFFFFFFull);  // 0..4
  const int n = sel == 0 ? 0 : (1 << (sel - 1));  // 0,1,2,4,8 value bytes
  const uint8_t header = sel ? (uint8_t)(mt | (0x17 + sel))
                             : (uint8_t)(mt | v);
  h = fnv1a_64_byte(h, header);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 8; ++k) {
    const uint8_t b = (uint8_t)(v >> (8 * (7 - k)));
    const uint64_t h2 = fnv1a_64_byte(h, b);
    h = (k >= 8 - n) ? h2 : h;
  }
  return h;
}

// A uint above 0xFFFFFFFF: header 0x1B (major 0) and eight value bytes,
// nothing to select.  The caller guarantees the range.
KVIDX_HD uint64_t fnv_cbor_u64_wide(uint64_t h, uint64_t v) {
  h = fnv1a_64_byte(h, 0x1B);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int s = 56; s >= 0; s -= 8) h = fnv1a_64_byte(h, (uint8_t)(v >> s));
  return h;
}

// Branchless chain link (bit-identical to chunk_hash; GPU hot path).
// The token loop is force-unrolled on device: a rolled loop makes hipcc
// read tok[] via gpr_idx (register-indexed) with a vmcnt(0) wait at the
// loop head, which both serializes the reads and drains any prefetched
// next-chunk loads (measured in the FNV chain kernel's ISA).
//
// wide_parent: the caller promises parent > 0xFFFFFFFF, which a chained
// parent (a 64-bit hash) is with probability 1 - 2^-32; the parent item
// is then nine straight steps in place of eight predicated ones.  On the
// device the flag must be uniform over the wave (k_fnv_chain_tr votes
// on it) so that taking it is a scalar branch.  Callers that run one
// chain on a single lane or per-lane event chains (the ingest kernels)
// pass false: they have no whole wave to vote with, and a per-lane
// branch would make the wave run both bodies.  Everything after the
// parent item is the same code either way.
template <typename TokT>
KVIDX_HD uint64_t chunk_hash_fast(uint64_t parent, const TokT* tokens,
                                  int n, bool wide_parent = false) {
  uint64_t h = FNV64_OFFSET;
  h = fnv1a_64_byte(h, 0x83);
  if (wide_parent)
    h = fnv_cbor_u64_wide(h, parent);
  else
    h = fnv_cbor_u64_branchless(h, parent, 0);
  // for a compile-time n the array header folds to constant bytes
  h = fnv_cbor_u32_branchless(h, (uint32_t)n, 4);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < n; ++i)
    h = fnv_cbor_u32_branchless(h, (uint32_t)tokens[i], 0);
  h = fnv1a_64_byte(h, 0xF6);
  return h;
}

// One chain link: FNV-64a(CBOR([parent, tokens[0..n), null])), streamed.
template <typename TokT>
KVIDX_HD uint64_t chunk_hash(uint64_t parent, const TokT* tokens, int n) {
  uint64_t h = FNV64_OFFSET;
  h = fnv1a_64_byte(h, 0x83);                    // array(3)
  h = fnv_cbor_uint(h, parent, 0);
  h = fnv_cbor_uint(h, (uint64_t)n, 4);          // tokens array header
  for (int i = 0; i < n; ++i) h = fnv_cbor_uint(h, (uint64_t)(uint32_t)tokens[i], 0);
  h = fnv1a_64_byte(h, 0xF6);                    // null
  return h;
}

// ---------------------------------------------------------------------
// SHA-256 chain link (hash_algo "sha256-cbor-64" / "sha256-cbor-64-low"):
// SHA-256 over the same canonical-CBOR payload, 64 digest bits kept.
// Native algo ids (utils/hashing.py NATIVE_ALGO_IDS is the one place
// that maps names to them):
//   0 fnv-64a            (everything above)
//   1 sha256-cbor-64     digest bytes 0..8  big-endian = state H0:H1
//   2 sha256-cbor-64-low digest bytes 24..32 big-endian = state H6:H7
//
// Two drivers share the byte packer, the CBOR item builders and the
// compression function:
//  - chunk_hash_sha256: streaming through one 16-word block buffer,
//    compressing whenever it fills (host ops and the GPU kernels whose
//    chains are not wave-dense);
//  - chunk_hash_sha256_wave: encodes the WHOLE padded payload into a
//    caller-provided word buffer first (an LDS column on the GPU), then
//    runs the compression for the wave-maximum block count with a
//    per-lane select - every lane compresses at the same time, so the 64
//    rounds never diverge (the read-path kernel k_sha_chain_tr).
// ---------------------------------------------------------------------

static constexpr int ALGO_FNV64A = 0;
static constexpr int ALGO_SHA256_HI = 1;
static constexpr int ALGO_SHA256_LOW = 2;

KVIDX_HD bool algo_valid(int64_t algo) { return algo >= 0 && algo <= 2; }
// First state word of the 64 bits an algo keeps.
KVIDX_HD constexpr int sha_digest_word(int algo) {
  return algo == ALGO_SHA256_LOW ? 6 : 0;
}

// Largest payload [parent, n tokens, null] in bytes, and the SHA block
// count it pads to (0x80 + 8 length bytes appended).
KVIDX_HD constexpr int sha_max_payload(int n) {
  return 1 + 9 + (n < 24 ? 1 : n <= 0xFF ? 2 : n <= 0xFFFF ? 3 : 5) + 5 * n +
         1;
}
KVIDX_HD constexpr int sha_blocks_for(int payload_bytes) {
  return (payload_bytes + 9 + 63) >> 6;
}

KVIDX_HD uint32_t sha_rotr(uint32_t x, int n) {
  return (x >> n) | (x << (32 - n));
}

// One SHA-256 block.  Rounds are fully unrolled on the device so the
// rolling 16-word schedule is indexed statically (a dynamically indexed
// w[] would live in scratch).
KVIDX_HD void sha256_compress(uint32_t st[8], uint32_t w[16]) {
  constexpr uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu,
      0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
      0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u,
      0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
      0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u,
      0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
      0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu,
      0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u,
      0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
      0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
      0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
      0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
  uint32_t e = st[4], f = st[5], g = st[6], h = st[7];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 64; ++i) {
    if (i >= 16) {
      const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
      w[i & 15] += (sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3)) +
                   w[(i - 7) & 15] +
                   (sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10));
    }
    const uint32_t t1 = h +
                        (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) +
                        ((e & f) ^ (~e & g)) + K[i] + w[i & 15];
    const uint32_t t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) +
                        ((a & b) ^ (a & c) ^ (b & c));
    h = g; g = f; f = e; e = d + t1;
    d = c; c = b; b = a; a = t1 + t2;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d;
  st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

KVIDX_HD void sha256_iv(uint32_t st[8]) {
  st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u;
  st[3] = 0xa54ff53au; st[4] = 0x510e527fu; st[5] = 0x9b05688cu;
  st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

// Canonical-CBOR unsigned (<= 32 bit) as a LEFT-aligned big-endian byte
// string in a u64 (header first); *len gets its 1..5 bytes.  Branchless.
KVIDX_HD uint64_t sha_cbor_u32_item(uint32_t v, uint8_t major, int* len) {
  const uint8_t mt = major << 5;
  const int sel = (v >= 24) + (v > 0xFF) + (v > 0xFFFF);  // 0..3
  const int n = sel == 3 ? 4 : sel;                       // value bytes
  const uint8_t header = sel ? (uint8_t)(mt | (0x17 + sel))
                             : (uint8_t)(mt | v);
  *len = 1 + n;
  // n == 0: the value lives in the header byte; v << 56 must not be OR-ed
  const uint64_t val = sel ? ((uint64_t)v << (56 - 8 * n)) : 0ull;
  return ((uint64_t)header << 56) | val;
}

// Item k of the padded-payload byte stream of one chain link, as a
// left-aligned byte string (<= 5 bytes) in a u64:
//   0: 0x83 + parent header   1/2: parent value, high / low <= 4 bytes
//   3: array(n) header        4..3+n: tokens   4+n: null (0xF6)
//   5+n: the SHA pad byte 0x80 (not part of the payload length)
// Branchless per item; with a compile-time k the selection folds away.
KVIDX_HD constexpr int sha_chunk_items(int n) { return n + 6; }

template <typename TokT>
KVIDX_HD uint64_t sha_chunk_item(int k, uint64_t parent, const TokT* tokens,
                                 int n, int* len) {
  if (k < 3) {
    const int sel = (parent >= 24) + (parent > 0xFF) + (parent > 0xFFFF) +
                    (parent > 0xFFFFFFFFull);            // 0..4
    const int nv = sel == 0 ? 0 : (1 << (sel - 1));      // 0,1,2,4,8
    if (k == 0) {
      const uint8_t ph = sel ? (uint8_t)(0x17 + sel) : (uint8_t)parent;
      *len = 2;
      return (0x83ull << 56) | ((uint64_t)ph << 48);
    }
    if (k == 1) {
      const int n_hi = nv == 8 ? 4 : 0;
      *len = n_hi;
      return n_hi ? (parent >> 32) << 32 : 0ull;
    }
    const int n_lo = nv == 8 ? 4 : nv;
    *len = n_lo;
    return n_lo ? (uint64_t)(uint32_t)parent << (64 - 8 * n_lo) : 0ull;
  }
  if (k == 3) return sha_cbor_u32_item((uint32_t)n, 4, len);
  if (k < 4 + n) return sha_cbor_u32_item((uint32_t)tokens[k - 4], 0, len);
  *len = 1;
  return (k == 4 + n ? 0xF6ull : 0x80ull) << 56;
}

// Big-endian byte packer.  acc holds the `fill` (< 4) pending bytes
// left-aligned; bits past them are zero.  put() leaves the next two
// words in hi/lo (lo possibly partial, zero-padded) and says how many of
// them (adv, 0..2) are complete.  Callers store BOTH words at their
// write index and advance by adv: a partial word is simply overwritten
// by its completed version, so there is no data-dependent store.
struct ShaPacker {
  uint64_t acc = 0;
  int fill = 0;
  int nbytes = 0;
  uint32_t hi = 0, lo = 0;
  // item: left-aligned bytes, len <= 5 (fill + len <= 8 fits acc)
  KVIDX_HD int put(uint64_t item, int len) {
    acc |= item >> (8 * fill);
    fill += len;
    nbytes += len;
    const int adv = fill >> 2;
    hi = (uint32_t)(acc >> 32);
    lo = (uint32_t)acc;
    acc = adv == 0 ? acc : adv == 1 ? (acc << 32) : 0ull;
    fill &= 3;
    return adv;
  }
};

// One chain link, streamed through a single block buffer:
// SHA-256(CBOR([parent, tokens[0..n), null])), returning state words
// digest_word:digest_word+1 as a big-endian u64.  The loop has ONE
// compression site; w[16..17] catch the word pair that straddles a block
// boundary and are carried down after the block is consumed.
template <typename TokT>
KVIDX_HD uint64_t chunk_hash_sha256(uint64_t parent, const TokT* tokens, int n,
                                    int digest_word) {
  uint32_t st[8];
  uint32_t w[18];
  w[16] = w[17] = 0;  // carried down before they are first written
  sha256_iv(st);
  ShaPacker p;
  const int n_items = sha_chunk_items(n);
  int widx = 0, k = 0;
  bool tail_done = false, finished = false;
  for (;;) {
    if (widx >= 16) {
      sha256_compress(st, w);
      w[0] = w[16];
      w[1] = w[17];
      widx -= 16;
      if (finished) break;
    }
    if (k < n_items) {
      int len;
      const uint64_t item = sha_chunk_item(k++, parent, tokens, n, &len);
      const int adv = p.put(item, len);
      w[widx] = p.hi;
      w[widx + 1] = p.lo;
      widx += adv;
    } else if (!tail_done) {
      widx += p.fill ? 1 : 0;  // the partial word is already in w[widx]
      tail_done = true;
    } else if (widx == 14) {   // 64-bit big-endian bit length
      w[14] = 0;
      w[15] = (uint32_t)(p.nbytes - 1) * 8u;  // minus the 0x80 pad byte
      widx = 16;
      finished = true;
    } else {
      w[widx++] = 0;
    }
  }
  uint64_t out = 0;
  for (int i = 0; i < 8; i += 2)  // static indices only (no st[] in scratch)
    if (i == digest_word) out = ((uint64_t)st[i] << 32) | st[i + 1];
  return out;
}

// Wave-convergent chain link.  buf (st(i, v) / ld(i)) must hold
// 16 * sha_blocks_for(sha_max_payload(n)) words private to this lane - an
// LDS column on the GPU.  Each lane first encodes its WHOLE padded
// payload, then the compression runs for the wave-maximum block count
// with a per-lane select dropping the blocks a lane does not have, so
// the 64 rounds never diverge.  any(p) is the wave-wide OR of p
// (identity on the host).  `active`: this lane's result is wanted (idle
// lanes compute and the caller discards).
template <typename TokT, class Buf, class AnyFn>
KVIDX_HD uint64_t chunk_hash_sha256_wave(uint64_t parent, const TokT* tokens,
                                         int n, int digest_word, Buf& buf,
                                         bool active, AnyFn any) {
  const int max_blocks = sha_blocks_for(sha_max_payload(n));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < max_blocks * 16; ++i) buf.st(i, 0u);
  ShaPacker p;
  int widx = 0;
  const int n_items = sha_chunk_items(n);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < n_items; ++k) {
    int len;
    const uint64_t item = sha_chunk_item(k, parent, tokens, n, &len);
    const int adv = p.put(item, len);
    buf.st(widx, p.hi);
    buf.st(widx + 1, p.lo);
    widx += adv;
  }
  const int payload = p.nbytes - 1;  // minus the 0x80 pad byte
  const int nblk = sha_blocks_for(payload);
  buf.st(nblk * 16 - 1, (uint32_t)payload * 8u);
  uint32_t st[8];
  sha256_iv(st);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int blk = 0; blk < max_blocks; ++blk) {
    const bool mine = blk < nblk;
    if (!any(active && mine)) break;
    uint32_t w[16], nx[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 16; ++i) w[i] = buf.ld(blk * 16 + i);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 8; ++i) nx[i] = st[i];
    sha256_compress(nx, w);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 8; ++i) st[i] = mine ? nx[i] : st[i];
  }
  uint64_t out = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 8; i += 2)
    if (i == digest_word) out = ((uint64_t)st[i] << 32) | st[i + 1];
  return out;
}

// Plain word buffer for the host build of chunk_hash_sha256_wave.
struct ShaHostBuf {
  uint32_t* p;
  KVIDX_HD void st(int i, uint32_t v) { p[i] = v; }
  KVIDX_HD uint32_t ld(int i) const { return p[i]; }
};
struct ShaHostAny {
  KVIDX_HD bool operator()(bool b) const { return b; }
};

// Compile-time chain policy used by the kernels and host ops.
template <int ALGO, typename TokT>
KVIDX_HD uint64_t chain_link(uint64_t parent, const TokT* tokens, int n) {
  if constexpr (ALGO == ALGO_FNV64A)
    return chunk_hash_fast(parent, tokens, n);
  else
    return chunk_hash_sha256(parent, tokens, n, sha_digest_word(ALGO));
}

KVIDX_HD uint32_t make_pod_entry(uint32_t pod_id, uint32_t tier) {
  return ((tier & 0xFu) << 24) | ((pod_id + 1) & 0x00FFFFFFu);
}

KVIDX_HD uint32_t pod_entry_id(uint32_t e) { return (e & 0x00FFFFFFu) - 1; }
KVIDX_HD uint32_t pod_entry_tier(uint32_t e) { return (e >> 24) & 0xFu; }

// Probe start position (golden-ratio scramble so clustered hashes spread).
KVIDX_HD uint64_t probe_start(uint64_t h, uint64_t cap_mask) {
  return (h * 0x9E3779B97F4A7C15ull) & cap_mask;
}

// Raw view of one table bundle (layout above); the arrays never alias.
struct Table {
  uint64_t* __restrict__ keys;
  uint32_t* __restrict__ meta;
  int32_t* __restrict__ stamp;
  uint32_t* __restrict__ pods;
  uint64_t* __restrict__ e_keys;
  uint32_t* __restrict__ e_meta;
  uint64_t* __restrict__ e_vals;
  uint64_t cap_mask;
  int pods_per_key;
};

// Slot of the live (occupied, not tombstoned) entry for (h, model) in a
// keys/meta pair - the main table or the engine map - or -1.  A never-used
// key word ends the probe chain.
KVIDX_HD int64_t probe_find(const uint64_t* __restrict__ keys,
                            const uint32_t* __restrict__ meta,
                            uint64_t cap_mask, uint64_t h, uint32_t model) {
  h = remap_hash(h);
  uint64_t s = probe_start(h, cap_mask);
  for (int t = 0; t < PROBE_MAX; ++t) {
    uint64_t i = (s + t) & cap_mask;
    uint64_t k = keys[i];
    if (k == 0) return -1;
    uint32_t m = meta[i];
    if ((m & META_OCC) && !(m & META_TOMB) && k == h &&
        (m & META_MODEL_MASK) == model)
      return (int64_t)i;
  }
  return -1;
}

// ---- purge by pod -----------------------------------------------------
// A purge bitmap is W 64-bit words; bit pid % 64 of word pid / 64 selects
// pod id pid.  Tier bits of an entry never take part.
KVIDX_HD bool purge_selects(const uint64_t* words, int W, uint32_t e) {
  const uint32_t pid = pod_entry_id(e);  // e == 0 -> 0xFFFFFFFF: no match
  return e != 0 && pid < (uint32_t)W * 64u && ((words[pid >> 6] >> (pid & 63)) & 1);
}
// Does a slot with meta word m take part in a purge for model_id
// (-1: every model)?  Tombstoned slots do: a stale entry left in one
// would come back when the key is resurrected.
KVIDX_HD bool purge_slot_eligible(uint32_t m, int64_t model_id) {
  return (m & META_OCC) &&
         (model_id < 0 || (int64_t)(m & META_MODEL_MASK) == model_id);
}

struct PurgeCounts {
  int64_t entries_cleared = 0;
  int64_t keys_tombstoned = 0;
};

// Host sweep: strip the selected pods from every eligible slot's pod set
// and tombstone each live slot that this call emptied.  stamp, keys and
// the engine map are untouched (the dev_remove_pods / cpu_evict stance).
// Single writer; k_purge_pods is the device twin.
inline PurgeCounts purge_pods_host(const Table& v, const uint64_t* words,
                                   int W, int64_t model_id) {
  PurgeCounts out;
  for (uint64_t i = 0; i <= v.cap_mask; ++i) {
    const uint32_t m = v.meta[i];
    if (!purge_slot_eligible(m, model_id)) continue;
    uint32_t* p = v.pods + i * (uint64_t)v.pods_per_key;
    int cleared = 0, left = 0;
    for (int k = 0; k < v.pods_per_key; ++k) {
      if (purge_selects(words, W, p[k])) {
        p[k] = 0;
        ++cleared;
      } else if (p[k] != 0) {
        ++left;
      }
    }
    out.entries_cleared += cleared;
    if (cleared && !left && !(m & META_TOMB)) {
      v.meta[i] = m | META_TOMB;
      ++out.keys_tombstoned;
    }
  }
  return out;
}

// ---- remap pod ids ----------------------------------------------------
// A remap gives every pod id below n a fate: kept, moved to another id, or
// dropped.  Both sweeps work from its 16-bit code table, codes[old] =
// new id + 1 and 0 = drop: 8 KB at MAX_PODS, which is what the kernel
// stages in LDS.
static constexpr int MAX_PODS = 4096;

// What entry e becomes under the map: e itself if it is empty, if its id
// lies past the map, or if the id maps to itself; 0 if the id is dropped;
// else the new id under e's own tier bits.  The one definition for the
// host sweep and k_remap_pods.
KVIDX_HD uint32_t remap_entry(uint32_t e, const uint16_t* codes, uint32_t n) {
  const uint32_t pid = pod_entry_id(e);  // e == 0 -> 0xFFFFFFFF: past n
  if (pid >= n) return e;
  const uint32_t c = codes[pid];
  return c ? ((e & 0xFF000000u) | c) : 0u;
}

// codes[0..n) from remap[0..n) (values -1..MAX_PODS-1, checked by the ops).
inline void remap_codes(const int32_t* remap, int n, uint16_t* codes) {
  for (int i = 0; i < n; ++i) codes[i] = (uint16_t)(remap[i] + 1);
}

struct RemapCounts {
  int64_t entries_moved = 0;
  int64_t entries_cleared = 0;
  int64_t keys_tombstoned = 0;
};

// Host sweep: rewrite every entry of every occupied slot (tombstoned ones
// too - purge_slot_eligible(m, -1)) by remap_entry, and tombstone each
// live slot that lost an entry to this call and kept none.  An injective
// map never puts one id into a row twice.  stamp, keys and the engine map
// are untouched.  Single writer; k_remap_pods is the device twin.
inline RemapCounts remap_pods_host(const Table& v, const int32_t* remap,
                                   int n) {
  uint16_t codes[MAX_PODS];
  remap_codes(remap, n, codes);
  RemapCounts out;
  for (uint64_t i = 0; i <= v.cap_mask; ++i) {
    const uint32_t m = v.meta[i];
    if (!purge_slot_eligible(m, -1)) continue;
    uint32_t* p = v.pods + i * (uint64_t)v.pods_per_key;
    int cleared = 0, left = 0;
    for (int k = 0; k < v.pods_per_key; ++k) {
      const uint32_t e = p[k];
      if (e == 0) continue;
      const uint32_t ne = remap_entry(e, codes, (uint32_t)n);
      if (ne == 0) {
        ++cleared;
      } else {
        ++left;
        out.entries_moved += ne != e;
      }
      if (ne != e) p[k] = ne;
    }
    out.entries_cleared += cleared;
    if (cleared && !left && !(m & META_TOMB)) {
      v.meta[i] = m | META_TOMB;
      ++out.keys_tombstoned;
    }
  }
  return out;
}

// Sharding: the main table holds only the keys a shard owns (the engine
// map is replicated on every shard).
KVIDX_HD bool owns_key(uint64_t h, int shard_id, int num_shards) {
  return num_shards <= 1 ||
         (int)(remap_hash(h) % (uint64_t)num_shards) == shard_id;
}

}  // namespace kvidx
