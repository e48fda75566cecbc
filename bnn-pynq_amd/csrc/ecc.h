// ecc.h -- a SEC-DED code for the 16-bit threshold memories, as an axis orthogonal to the hardening scheme
// (bnn_mi355x_ecc_exposure_campaigns; the storage and the upsets: mem_org.h, "coded threshold memories").
//
// The code is the project's own model, not the fork's (which has none): parity unpinned, like the voter and the
// activation faults.  It is what block RAM ECC is: a Hamming code with an overall parity bit, here Hamming(21,16) --
// 16 data bits and 6 check bits per threshold element.
//   Code word positions are 1 ... 21.  Positions 1, 2, 4, 8, 16 hold check bits c0 ... c4; the other positions, in
//   increasing order (3, 5, 6, 7, 9, ..., 15, 17, ..., 21), hold data bits 0 ... 15.  c_j is the XOR of the data bits
//   whose position has bit j set; c5 is the XOR of all 16 data bits and c0 ... c4 (every code word has even weight).
//   Decode (stored data d, stored check c): s = (encode(d) ^ c) & 31, P = parity(d) ^ parity(c).
//     s = 0, P = 0                          status 0, data d
//     P = 1, s = 0 or a power of two        status 1 (corrected: a check bit was hit), data d
//     P = 1, s a data position              status 1, data d with that data bit flipped
//     P = 1, s = 22 ... 31                  status 2 (detected, uncorrectable), data d as stored
//     P = 0, s != 0                         status 2, data d as stored
//   Every single error of the 22 bits is restored; none of the 231 double errors is miscorrected (status 2, the data as
//   stored); of the 1 540 triples 1 052 are accepted as a correction (the data then wrong) and 488 detected.
// The code is linear: status and corrected bit depend on the error pattern (data mask dm, check mask cm) alone --
//     decode(d ^ dm, encode(d) ^ cm) = (status of decode(dm, cm), d ^ data of decode(dm, cm)),
// which is how the kernel (k_emem_noise_t) uses it: it decodes the accumulated hit masks, never a stored word.
// A REPAIR (ecc_repair below; the exposure campaigns' repair scrub: mem_org.h, "repair scrubs") reads a stored word,
// decodes it and, with status 1, writes the delivered data d' and encode(d') back; with status 0 or 2 it writes nothing.
// By the same linearity that is a rule on error patterns, and the one k_repair_state applies to its hit masks:
//     (dm, cm) -> (m, encode(m)) where decode(dm, cm) = (1, m), else (dm, cm) unchanged
// -- a stored word d ^ dm, encode(d) ^ cm becomes d ^ m, encode(d ^ m) = encode(d) ^ encode(m).  The decoder flips exactly
// one of the 22 positions, so what a status-1 repair stores is always a valid code word: a corrected single returns to
// the loaded word (m = 0), an accepted triple becomes a clean-looking wrong one (m != 0, status 0 from then on) that no
// later repair touches.  The delivered data is d' before and after.
//
// Two limits.  WEIGHTS are not coded BY THIS CODE: their memory words are SIMD * wbits wide (1 ... 64 bits in the fold
// tables) and no per-word code makes sense over them; the code over them is the one that lies over the memory 64 data
// bits at a time, whatever the word width -- wecc.h, a `weight_code` axis of its own.  The 24-bit threshold memory
// of CNV LAYER 0 is not coded: a fault there passes through the reference's integer-part read-back (apply_fault), which
// rewrites the whole word, and no code word survives that; layer 0 keeps the uncoded host route, and a study that wants
// it out of the picture sets its rates to 0.  A scrub is a full rewrite (data and check words) or a repair (above).
#pragma once
#include <stdint.h>

#ifndef BNN_HD
#define BNN_HD
#endif

namespace bnn {

enum : int { EC_NONE = 0, EC_SECDED = 1 };
constexpr int kEccDataBits = 16, kEccCheckBits = 6;

BNN_HD inline uint32_t ecc_parity(uint32_t v) { return (uint32_t)__builtin_popcount(v) & 1u; }

// the 6 check bits of a 16-bit data word.  The masks: data bit k sits at position 3, 5, 6, 7, 9 ... 15, 17 ... 21
BNN_HD inline uint32_t ecc_encode(uint32_t data) {
  const uint32_t d = data & 0xFFFFu;
  const uint32_t c = ecc_parity(d & 0xAD5Bu) | ecc_parity(d & 0x366Du) << 1 | ecc_parity(d & 0xC78Eu) << 2 | ecc_parity(d & 0x07F0u) << 3 |
                     ecc_parity(d & 0xF800u) << 4;
  return c | (ecc_parity(d) ^ ecc_parity(c)) << 5;
}

// status 0 clean, 1 corrected, 2 detected; *out the data the decoder delivers.  With (data, check) an error pattern
// (dm, cm), *out is the error that remains in the delivered data.
BNN_HD inline int ecc_decode(uint32_t data, uint32_t check, uint32_t *out) {
  const uint32_t d = data & 0xFFFFu, c = check & 0x3Fu;
  const uint32_t s = (ecc_encode(d) ^ c) & 31u, P = ecc_parity(d) ^ ecc_parity(c);
  *out = d;
  if (P == 0) return s == 0 ? 0 : 2;
  if ((s & (s - 1)) == 0) return 1;  // (0: the overall parity bit itself; a power of two: one of c0 ... c4)
  if (s > 21) return 2;
  uint32_t hb = 0;  // position s holds data bit s - (the powers of two below s) - 1
  for (uint32_t t = s; t >>= 1;) hb++;
  *out = d ^ (1u << (s - hb - 2));
  return 1;
}

// what a repair leaves stored of (data, check), and the decode status: status 1 the delivered data and its check bits,
// else the word as it was.  With an error pattern (dm, cm): the pattern that remains.
BNN_HD inline int ecc_repair(uint32_t data, uint32_t check, uint32_t *out_data, uint32_t *out_check) {
  uint32_t d;
  const int status = ecc_decode(data, check, &d);
  *out_data = status == 1 ? d : (data & 0xFFFFu);
  *out_check = status == 1 ? ecc_encode(d) : (check & 0x3Fu);
  return status;
}

}  // namespace bnn
