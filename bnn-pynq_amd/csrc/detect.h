// Host half of the detections (bnn_mi355x_detect_windows*, bnn_mi355x_detect_clip): the windows of a frame and their scores
// become a short list of boxes -- threshold, order, cap, greedy non-maximum suppression ("Detections").
//
// The model is the project's own (the reference draws every window that fires): parity unpinned.  It is pure integer, so
// the kernels (csrc/detect_kernels.hip) are pinned to it byte for byte; tests/detect_ref.py restates it in plain numpy.
//   class     by_score = 0: the decode's class of the window -- the first strict maximum over the first number_class
//             scores, floored at 0 (scores <= 0 never beat class 0; k_fclast* in kernels.hip).  by_score = 1: class_mask has
//             exactly one bit k, and the class is k whatever the argmax.
//   candidate the class is in class_mask and score[class] > min_score.
//   order     score descending, then window index ascending; only the first max_candidates take part, n_candidates
//             counts all that passed.
//   suppress  walk the order, keep a candidate unless an already kept one OF ITS CLASS has
//             inter * iou_den > iou_num * union (64-bit, strict); stop after max_det kept.
//   output    per kept candidate 8 ints: left, upper, right, lower, class, score, window index, right - left.  The rows
//             of a frame past its count are zero.
// Host-only but for detect_suppresses, which the kernel shares (BNN_HD, as ecc.h and wecc.h).  No HIP in this file.
#pragma once
#include <stdint.h>

#include <string>

#ifndef BNN_HD
#define BNN_HD
#endif

namespace bnn {

// Limits (include/bnn_mi355x.h states them)
constexpr int kDetectMaxCandidates = 4096;
constexpr int kDetectMaxCoord = 65535;
constexpr long kDetectMaxWindows = 1 << 20;  // of all frames of one call (the scan's limit: an index has 20 bits)
constexpr int kDetectMaxFrames = 4096;
constexpr int kDetectMaxIouDen = 65536;
constexpr int kDetectFields = 8;

struct DetectOpts {  // (bnn_mi355x_detect_opts)
  uint64_t class_mask;
  int by_score, min_score, iou_num, iou_den, max_candidates, max_det;
};

// Whether a kept box a suppresses box b: IoU(a, b) > num / den, in integers.  Coordinates are 0 .. 65535 with left < right
// and upper < lower: inter and union stay below 2^33, the products below 2^50.  num == den never suppresses.
BNN_HD inline bool detect_suppresses(int al, int au, int ar, int ab, int bl, int bu, int br, int bb, int num, int den) {
  const int iw = (ar < br ? ar : br) - (al > bl ? al : bl), ih = (ab < bb ? ab : bb) - (au > bu ? au : bu);
  if (iw <= 0 || ih <= 0) return false;
  const int64_t inter = (int64_t)iw * ih;
  const int64_t uni = (int64_t)(ar - al) * (ab - au) + (int64_t)(br - bl) * (bb - bu) - inter;
  return inter * (int64_t)den > (int64_t)num * uni;
}

// The decode's class of one window's scores (restated from k_fclast*: the reference's loop)
inline int detect_decode_class(const int *scores, int number_class) {
  int best = 0, bestv = 0;
  for (int c = 0; c < number_class; c++)
    if (scores[c] > bestv) { bestv = scores[c]; best = c; }
  return best;
}

// Empty when the options can be used, else the message for last_error (`what`: the entry point's name), naming the field
std::string validate_detect_opts(const char *what, int number_class, const DetectOpts *opts);
// The same for a whole detect_windows call: the counts, the pointers, the options, every box and every score
std::string validate_detect(const char *what, const int *boxes, long n, const int *scores, int frames, int number_class, const DetectOpts *opts,
                            const int *dets, const int *counts, const int *n_candidates);

// The model on validated arguments.  scores: [frames][n][number_class]; dets: [frames][max_det][8]; counts, n_candidates: [frames]
void detect_windows(const int *boxes, long n, const int *scores, int frames, int number_class, const DetectOpts &opts, int *dets, int *counts,
                    int *n_candidates);

}  // namespace bnn
