// The detections' model on the host (detect.h): validation and the reference statement the kernels are pinned to.
#include "detect.h"

#include <algorithm>
#include <vector>

namespace bnn {

std::string validate_detect_opts(const char *what, int number_class, const DetectOpts *opts) {
  const std::string w = std::string(what) + ": ";
  if (!opts) return w + "opts is null";
  if (number_class < 1 || number_class > 64) return w + "number_class must be in 1..64";
  const DetectOpts &o = *opts;
  if (o.class_mask == 0) return w + "class_mask is 0: no class is wanted";
  if (number_class < 64 && (o.class_mask >> number_class) != 0)
    return w + "class_mask names a class at or above number_class (" + std::to_string(number_class) + ")";
  if (o.by_score != 0 && o.by_score != 1) return w + "by_score must be 0 or 1";
  if (o.by_score && (o.class_mask & (o.class_mask - 1)) != 0) return w + "by_score needs a class_mask of exactly one bit";
  if (o.iou_den < 1 || o.iou_den > kDetectMaxIouDen) return w + "iou_den must be in 1.." + std::to_string(kDetectMaxIouDen);
  if (o.iou_num < 0 || o.iou_num > o.iou_den) return w + "iou_num must be in 0..iou_den";
  if (o.max_candidates < 1 || o.max_candidates > kDetectMaxCandidates)
    return w + "max_candidates must be in 1.." + std::to_string(kDetectMaxCandidates);
  if (o.max_det < 1 || o.max_det > o.max_candidates) return w + "max_det must be in 1..max_candidates";
  return "";
}

std::string validate_detect(const char *what, const int *boxes, long n, const int *scores, int frames, int number_class, const DetectOpts *opts,
                            const int *dets, const int *counts, const int *n_candidates) {
  const std::string w = std::string(what) + ": ";
  if (!boxes) return w + "boxes is null";
  if (!scores) return w + "scores is null";
  if (!dets) return w + "dets is null";
  if (!counts) return w + "counts is null";
  if (!n_candidates) return w + "n_candidates is null";
  if (frames < 1 || frames > kDetectMaxFrames) return w + "frames must be in 1.." + std::to_string(kDetectMaxFrames);
  if (n < 1 || n > kDetectMaxWindows || n * frames > kDetectMaxWindows)
    return w + "n must be 1 or more, and n x frames at most " + std::to_string(kDetectMaxWindows);
  const std::string bad = validate_detect_opts(what, number_class, opts);
  if (!bad.empty()) return bad;
  for (long i = 0; i < n; i++) {
    const int *b = boxes + 4 * i;
    if (b[0] < 0 || b[1] < 0 || b[2] > kDetectMaxCoord || b[3] > kDetectMaxCoord || b[0] >= b[2] || b[1] >= b[3])
      return w + "boxes[" + std::to_string(i) + "] is empty, inverted or outside 0.." + std::to_string(kDetectMaxCoord);
  }
  const long total = n * frames * number_class;
  for (long i = 0; i < total; i++)
    if (scores[i] < -32768 || scores[i] > 32767) return w + "scores[" + std::to_string(i) + "] is outside int16";
  return "";
}

void detect_windows(const int *boxes, long n, const int *scores, int frames, int number_class, const DetectOpts &o, int *dets, int *counts,
                    int *n_candidates) {
  struct Cand { int score, cls; long idx; };
  int only = 0;
  while (o.by_score && !((o.class_mask >> only) & 1)) only++;
  std::vector<Cand> cand;
  std::vector<int> kept;
  for (int f = 0; f < frames; f++) {
    const int *sc = scores + (size_t)f * n * number_class;
    int *out = dets + (size_t)f * o.max_det * kDetectFields;
    std::fill(out, out + (size_t)o.max_det * kDetectFields, 0);
    cand.clear();
    for (long i = 0; i < n; i++) {
      const int *s = sc + (size_t)i * number_class;
      const int cls = o.by_score ? only : detect_decode_class(s, number_class);
      if (((o.class_mask >> cls) & 1) && s[cls] > o.min_score) cand.push_back({s[cls], cls, i});
    }
    n_candidates[f] = (int)cand.size();
    // (the candidates are in index order: a stable sort by score keeps ties by index)
    std::stable_sort(cand.begin(), cand.end(), [](const Cand &a, const Cand &b) { return a.score > b.score; });
    if (cand.size() > (size_t)o.max_candidates) cand.resize((size_t)o.max_candidates);
    kept.clear();
    for (size_t c = 0; c < cand.size() && (int)kept.size() < o.max_det; c++) {
      const int *b = boxes + 4 * cand[c].idx;
      bool alive = true;
      for (size_t k = 0; k < kept.size() && alive; k++) {
        const Cand &a = cand[(size_t)kept[k]];
        const int *ab = boxes + 4 * a.idx;
        if (a.cls == cand[c].cls && detect_suppresses(ab[0], ab[1], ab[2], ab[3], b[0], b[1], b[2], b[3], o.iou_num, o.iou_den)) alive = false;
      }
      if (!alive) continue;
      int *d = out + kept.size() * kDetectFields;
      d[0] = b[0]; d[1] = b[1]; d[2] = b[2]; d[3] = b[3];
      d[4] = cand[c].cls; d[5] = cand[c].score; d[6] = (int)cand[c].idx; d[7] = b[2] - b[0];
      kept.push_back((int)c);
    }
    counts[f] = (int)kept.size();
  }
}

}  // namespace bnn
