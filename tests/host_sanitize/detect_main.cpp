// Stand-alone driver for tests/test_host_sanitize_detect.py: the host-only code of the detections (csrc/detect.cpp:
// validation and the model) under AddressSanitizer + UBSan.  Seeded random cases on exactly-sized vectors -- n <= 200,
// scores drawn from four values so that ties are everywhere, random options -- with the invariants of every answer, then
// the extremes: coordinates 65535, iou_den 65536, n = 1, the largest and smallest scores, and the refusals.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "detect.h"

using namespace bnn;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

// runs one validated case on exactly-sized outputs and checks what every answer must satisfy
static int run_case(const std::vector<int> &boxes, const std::vector<int> &scores, int frames, int ncls, const DetectOpts &o) {
  const long n = (long)boxes.size() / 4;
  std::vector<int> dets((size_t)frames * o.max_det * kDetectFields, -7), counts((size_t)frames, -7), ncand((size_t)frames, -7);
  CHECK(validate_detect("t", boxes.data(), n, scores.data(), frames, ncls, &o, dets.data(), counts.data(), ncand.data()).empty());
  detect_windows(boxes.data(), n, scores.data(), frames, ncls, o, dets.data(), counts.data(), ncand.data());
  for (int f = 0; f < frames; f++) {
    CHECK(counts[f] >= 0 && counts[f] <= o.max_det && ncand[f] >= counts[f] && ncand[f] <= n);
    CHECK((ncand[f] > 0) == (counts[f] > 0));
    const int *d = dets.data() + (size_t)f * o.max_det * kDetectFields;
    for (int k = 0; k < o.max_det; k++) {
      const int *r = d + k * kDetectFields;
      if (k >= counts[f]) {
        for (int j = 0; j < kDetectFields; j++) CHECK(r[j] == 0);
        continue;
      }
      const long i = r[6];
      CHECK(i >= 0 && i < n && r[0] == boxes[4 * i] && r[1] == boxes[4 * i + 1] && r[2] == boxes[4 * i + 2] && r[3] == boxes[4 * i + 3]);
      CHECK(r[7] == r[2] - r[0] && ((o.class_mask >> r[4]) & 1) && r[5] > o.min_score);
      CHECK(r[5] == scores[((size_t)f * n + i) * ncls + r[4]]);
      if (k) CHECK(r[-kDetectFields + 5] > r[5] || (r[-kDetectFields + 5] == r[5] && r[-kDetectFields + 6] < r[6]));  // the order
      for (int e = 0; e < k; e++) {  // no kept candidate of its class suppresses it
        const int *a = d + e * kDetectFields;
        CHECK(a[4] != r[4] || !detect_suppresses(a[0], a[1], a[2], a[3], r[0], r[1], r[2], r[3], o.iou_num, o.iou_den));
      }
    }
  }
  return 0;
}

int main() {
  std::mt19937 rng(2024);
  auto below = [&](int n) { return (int)(rng() % (uint32_t)n); };
  for (int c = 0; c < 200; c++) {
    const int n = 1 + below(200), frames = 1 + below(3), ncls = 1 + below(8);
    std::vector<int> boxes((size_t)n * 4), scores((size_t)frames * n * ncls);
    for (int i = 0; i < n; i++) {
      const int l = below(60), u = below(60);
      boxes[4 * i] = l; boxes[4 * i + 1] = u; boxes[4 * i + 2] = l + 1 + below(40); boxes[4 * i + 3] = u + 1 + below(40);
    }
    int values[4];
    for (int &v : values) v = below(640) - 40;
    for (int &s : scores) s = values[below(4)];
    DetectOpts o{};
    o.by_score = below(2);
    o.class_mask = o.by_score ? (uint64_t)1 << below(ncls) : (uint64_t)(1 + below((1 << ncls) - 1));
    o.min_score = below(5) ? values[below(4)] - below(2) : -32769;
    o.iou_den = 1 + below(kDetectMaxIouDen);
    o.iou_num = below(o.iou_den + 1);
    const int caps[5] = {1, 2, 7, 64, kDetectMaxCandidates};
    o.max_candidates = caps[below(5)];
    o.max_det = 1 + below(o.max_candidates < 80 ? o.max_candidates : 80);
    if (run_case(boxes, scores, frames, ncls, o)) return 1;
  }

  // the extremes: the largest coordinates and denominator (the products of detect_suppresses near their bound), n = 1
  {
    DetectOpts o{1, 0, -32769, kDetectMaxIouDen - 1, kDetectMaxIouDen, kDetectMaxCandidates, kDetectMaxCandidates};
    const std::vector<int> boxes = {0, 0, kDetectMaxCoord, kDetectMaxCoord, 1, 1, kDetectMaxCoord, kDetectMaxCoord,
                                    kDetectMaxCoord - 1, kDetectMaxCoord - 1, kDetectMaxCoord, kDetectMaxCoord, 0, 0, kDetectMaxCoord, kDetectMaxCoord};
    if (run_case(boxes, {32767, 32767, -32768, 5}, 1, 1, o)) return 1;
    // IoU 65534^2 / 65535^2 = 1 - 2 / 65535 + ...: between 65533 / 65536 and 65535 / 65536
    CHECK(detect_suppresses(0, 0, 65535, 65535, 1, 1, 65535, 65535, 65533, 65536));
    CHECK(!detect_suppresses(0, 0, 65535, 65535, 1, 1, 65535, 65535, 65535, 65536));
    CHECK(!detect_suppresses(0, 0, 65535, 65535, 1, 1, 65535, 65535, 65536, 65536));  // num == den never suppresses
    CHECK(!detect_suppresses(0, 0, 65535, 65535, 0, 0, 65535, 65535, 65536, 65536));
    CHECK(detect_suppresses(0, 0, 65535, 65535, 0, 0, 65535, 65535, 65535, 65536));
    CHECK(!detect_suppresses(0, 0, 10, 10, 10, 0, 20, 10, 0, 1));  // touching boxes do not overlap
    CHECK(detect_suppresses(0, 0, 32, 32, 4, 0, 36, 32, 50971, 65536) && !detect_suppresses(0, 0, 32, 32, 4, 0, 36, 32, 7, 9));
    o.max_candidates = o.max_det = 1;
    if (run_case({0, 0, 1, 1}, {-32768}, 1, 1, o)) return 1;
    o.class_mask = (uint64_t)1 << 63;
    o.by_score = 1;
    std::vector<int> wide(64, 0);
    wide[63] = 9;
    if (run_case({5, 5, 6, 6}, wide, 1, 64, o)) return 1;
  }

  // the refusals: each names its argument
  {
    const int box[4] = {0, 0, 4, 4}, score[2] = {1, 2};
    int out[16] = {}, cnt[1], nc[1];
    const DetectOpts good{0b11, 0, 0, 1, 2, 4, 2};
    CHECK(validate_detect("t", box, 1, score, 1, 2, &good, out, cnt, nc).empty());
    CHECK(has(validate_detect("t", nullptr, 1, score, 1, 2, &good, out, cnt, nc), "boxes"));
    CHECK(has(validate_detect("t", box, 1, nullptr, 1, 2, &good, out, cnt, nc), "scores"));
    CHECK(has(validate_detect("t", box, 1, score, 1, 2, nullptr, out, cnt, nc), "opts"));
    CHECK(has(validate_detect("t", box, 1, score, 1, 2, &good, nullptr, cnt, nc), "dets"));
    CHECK(has(validate_detect("t", box, 1, score, 1, 2, &good, out, nullptr, nc), "counts"));
    CHECK(has(validate_detect("t", box, 1, score, 1, 2, &good, out, cnt, nullptr), "n_candidates"));
    CHECK(has(validate_detect("t", box, 0, score, 1, 2, &good, out, cnt, nc), "n must"));
    CHECK(has(validate_detect("t", box, kDetectMaxWindows + 1, score, 1, 2, &good, out, cnt, nc), "n must"));
    CHECK(has(validate_detect("t", box, kDetectMaxWindows, score, 2, 2, &good, out, cnt, nc), "n must"));
    CHECK(has(validate_detect("t", box, 1, score, 0, 2, &good, out, cnt, nc), "frames"));
    CHECK(has(validate_detect("t", box, 1, score, kDetectMaxFrames + 1, 2, &good, out, cnt, nc), "frames"));
    CHECK(has(validate_detect("t", box, 1, score, 1, 0, &good, out, cnt, nc), "number_class"));
    CHECK(has(validate_detect("t", box, 1, score, 1, 65, &good, out, cnt, nc), "number_class"));
    auto with = [&](void (*change)(DetectOpts &)) { DetectOpts o = good; change(o); return validate_detect_opts("t", 2, &o); };
    CHECK(has(with([](DetectOpts &o) { o.class_mask = 0; }), "class_mask"));
    CHECK(has(with([](DetectOpts &o) { o.class_mask = 0b100; }), "class_mask"));
    CHECK(has(with([](DetectOpts &o) { o.by_score = 1; }), "by_score"));
    CHECK(has(with([](DetectOpts &o) { o.by_score = -1; }), "by_score"));
    CHECK(has(with([](DetectOpts &o) { o.iou_num = 3; }), "iou_num"));
    CHECK(has(with([](DetectOpts &o) { o.iou_num = -1; }), "iou_num"));
    CHECK(has(with([](DetectOpts &o) { o.iou_den = 0; }), "iou_den"));
    CHECK(has(with([](DetectOpts &o) { o.iou_den = kDetectMaxIouDen + 1; }), "iou_den"));
    CHECK(has(with([](DetectOpts &o) { o.max_candidates = 0; }), "max_candidates"));
    CHECK(has(with([](DetectOpts &o) { o.max_candidates = kDetectMaxCandidates + 1; }), "max_candidates"));
    CHECK(has(with([](DetectOpts &o) { o.max_det = 0; }), "max_det"));
    CHECK(has(with([](DetectOpts &o) { o.max_det = 5; }), "max_det"));
    CHECK(with([](DetectOpts &o) { o.by_score = 1; o.class_mask = 0b10; }).empty());
    DetectOpts all = good;
    all.class_mask = ~(uint64_t)0;
    CHECK(validate_detect_opts("t", 64, &all).empty() && has(validate_detect_opts("t", 63, &all), "class_mask"));
    const int bad_boxes[6][4] = {{4, 0, 4, 4}, {5, 0, 4, 4}, {0, 4, 4, 4}, {-1, 0, 4, 4}, {0, 0, 65536, 4}, {0, 0, 4, 65536}};
    for (const auto &b : bad_boxes) CHECK(has(validate_detect("t", b, 1, score, 1, 2, &good, out, cnt, nc), "boxes[0]"));
    const int big[2] = {1, 32768}, small[2] = {-32769, 1};
    CHECK(has(validate_detect("t", box, 1, big, 1, 2, &good, out, cnt, nc), "scores[1]"));
    CHECK(has(validate_detect("t", box, 1, small, 1, 2, &good, out, cnt, nc), "scores[0]"));
  }
  std::printf("detect sanitize run ok\n");
  return 0;
}
