// wecc.h -- a SEC-DED (72,64) code for the WEIGHT memories of the layers >= 1, as a third axis (`weight_code`) next to the
// hardening scheme and the threshold code of ecc.h (bnn_mi355x_wecc_exposure_campaigns; the storage and the upsets:
// mem_org.h, "coded weight memories").
//
// The code is the project's own model, not the fork's (which has none): parity unpinned, like the voter, the threshold
// code and the repair.  It is what block RAM ECC is: 64 data bits plus 8 check bits, laid over the memory whatever the
// logical word width -- Hamming(71,64) plus an overall parity bit.
//   Code word positions are 1 ... 71.  Positions 1, 2, 4, 8, 16, 32, 64 hold check bits c0 ... c6; the other positions,
//   in increasing order (3, 5, 6, 7, 9, ..., 15, 17, ..., 31, 33, ..., 63, 65, ..., 71), hold data bits 0 ... 63.  c_j is
//   the XOR of the data bits whose position has bit j set; c7 is the XOR of all 64 data bits and c0 ... c6 (every code
//   word has even weight).
//   Decode (stored data d, stored check c): s = (encode(d) ^ c) & 127, P = parity(d) ^ parity(c).
//     s = 0, P = 0                          status 0, data d
//     P = 1, s = 0 or a power of two        status 1 (corrected: a check bit was hit), data d
//     P = 1, s a data position              status 1, data d with that data bit flipped
//     P = 1, s = 72 ... 127                 status 2 (detected, uncorrectable), data d as stored
//     P = 0, s != 0                         status 2, data d as stored
//   Every single error of the 72 bits is restored; none of the 2 556 double errors is miscorrected (status 2, the data as
//   stored); a triple is either accepted as a correction (the data then wrong) or detected.
// The code is linear: status and corrected bit depend on the error pattern (data mask dm, check mask cm) alone --
//     decode(d ^ dm, encode(d) ^ cm) = (status of decode(dm, cm), d ^ data of decode(dm, cm)),
// which is how the kernel (k_wmem_noise_w) uses it: it decodes the accumulated hit masks, never a stored word.
// A REPAIR (wecc_repair below; mem_org.h, "repair scrubs") reads a stored word, decodes it and, with status 1, writes the
// delivered data d' and encode(d') back; with status 0 or 2 it writes nothing.  On error patterns (k_wrepair_state):
//     (dm, cm) -> (m, encode(m)) where decode(dm, cm) = (1, m), else (dm, cm) unchanged.
// The decoder flips exactly one of the 72 positions, so what a status-1 repair stores is always a valid code word: a
// corrected single returns to the loaded word (m = 0), an accepted triple becomes a clean-looking wrong one (m != 0,
// status 0 from then on) that no later repair touches.  The delivered data is d' before and after.
#pragma once
#include <stdint.h>

#ifndef BNN_HD
#define BNN_HD
#endif

namespace bnn {

enum : int { WC_NONE = 0, WC_SECDED = 1 };
constexpr int kWeccDataBits = 64, kWeccCheckBits = 8;

// the data bits that check bit j covers: data bit k sits at the k-th position of 1 ... 71 that is no power of two
constexpr uint64_t wecc_mask(int j) {
  uint64_t m = 0;
  int k = 0;
  for (int pos = 1; pos <= 71; pos++) {
    if ((pos & (pos - 1)) == 0) continue;
    if ((pos >> j) & 1) m |= 1ull << k;
    k++;
  }
  return m;
}

BNN_HD inline uint32_t wecc_parity(uint64_t v) { return (uint32_t)__builtin_popcountll(v) & 1u; }

// the 8 check bits of a 64-bit data word
BNN_HD inline uint32_t wecc_encode(uint64_t d) {
  constexpr uint64_t m0 = wecc_mask(0), m1 = wecc_mask(1), m2 = wecc_mask(2), m3 = wecc_mask(3), m4 = wecc_mask(4), m5 = wecc_mask(5),
                     m6 = wecc_mask(6);
  const uint32_t c = wecc_parity(d & m0) | wecc_parity(d & m1) << 1 | wecc_parity(d & m2) << 2 | wecc_parity(d & m3) << 3 |
                     wecc_parity(d & m4) << 4 | wecc_parity(d & m5) << 5 | wecc_parity(d & m6) << 6;
  return c | (wecc_parity(d) ^ wecc_parity(c)) << 7;
}

// status 0 clean, 1 corrected, 2 detected; *out the data the decoder delivers.  With (data, check) an error pattern
// (dm, cm), *out is the error that remains in the delivered data.
BNN_HD inline int wecc_decode(uint64_t data, uint32_t check, uint64_t *out) {
  const uint32_t c = check & 0xFFu;
  const uint32_t s = (wecc_encode(data) ^ c) & 127u, P = wecc_parity(data) ^ wecc_parity(c);
  *out = data;
  if (P == 0) return s == 0 ? 0 : 2;
  if ((s & (s - 1)) == 0) return 1;  // (0: the overall parity bit itself; a power of two: one of c0 ... c6)
  if (s > 71) return 2;
  uint32_t hb = 0;  // position s holds data bit s - (the powers of two below s) - 1
  for (uint32_t t = s; t >>= 1;) hb++;
  *out = data ^ (1ull << (s - hb - 2));
  return 1;
}

// what a repair leaves stored of (data, check), and the decode status: status 1 the delivered data and its check bits,
// else the word as it was.  With an error pattern (dm, cm): the pattern that remains.
BNN_HD inline int wecc_repair(uint64_t data, uint32_t check, uint64_t *out_data, uint32_t *out_check) {
  uint64_t d;
  const int status = wecc_decode(data, check, &d);
  *out_data = status == 1 ? d : data;
  *out_check = status == 1 ? wecc_encode(d) : (check & 0xFFu);
  return status;
}

}  // namespace bnn
