// Stand-alone driver for tests/test_host_sanitize_components.py: the host-only model of find_glyphs (csrc/components.cpp)
// under AddressSanitizer + UBSan.  Degenerate sizes, reach 16 at every border, cap 1, a picture that is all ink, row
// strides, every optional output on and off, and the validation.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "components.h"

using namespace bnn;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

// runs the whole host statement on exactly-sized buffers (the sanitizer sees any byte past them) and checks what every
// caller relies on: boxes inside the picture, counts that add up, labels below the number returned
static int run(const std::vector<uint8_t> &plane, int w, int h, long stride, const FindOpts &f, int cap, long *total_out = nullptr) {
  const size_t returned_max = (size_t)cap < max_components(w, h) ? (size_t)cap : max_components(w, h);
  for (int outputs = 0; outputs < 4; outputs++) {
    std::vector<int> boxes(returned_max * 4 + 1, -7), counts(returned_max + 1, -7);
    std::vector<int32_t> labels((size_t)w * h, -7);
    const long total = find_components_host(plane.data(), w, h, stride, f, boxes.data(), (outputs & 1) ? counts.data() : nullptr,
                                            (outputs & 2) ? labels.data() : nullptr, cap);
    CHECK(total >= 0 && (size_t)total <= max_components(w, h));
    const long n = total < cap ? total : cap;
    CHECK(boxes[(size_t)n * 4] == -7 && counts[(size_t)n] == -7);
    long ink = 0;
    const size_t row = stride ? (size_t)stride : (size_t)w;
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) ink += plane[(size_t)y * row + x] < f.ink_level;
    long counted = 0;
    for (long k = 0; k < n; k++) {
      const int *b = &boxes[(size_t)k * 4];
      CHECK(b[0] >= 0 && b[1] >= 0 && b[0] < b[2] && b[1] < b[3] && b[2] <= w && b[3] <= h);
      if (outputs & 1) {
        CHECK(counts[(size_t)k] >= f.min_pixels && (long)counts[(size_t)k] <= (long)(b[2] - b[0]) * (b[3] - b[1]));
        counted += counts[(size_t)k];
      }
    }
    if ((outputs & 1) && total <= cap && f.min_pixels == 1) CHECK(counted == ink);
    if (outputs & 2) {
      long labelled = 0;
      for (size_t p = 0; p < labels.size(); p++) {
        CHECK(labels[p] >= -1 && labels[p] < n);
        labelled += labels[p] >= 0;
        if (labels[p] >= 0) {
          const int x = (int)(p % (size_t)w), y = (int)(p / (size_t)w), *b = &boxes[(size_t)labels[p] * 4];
          CHECK(x >= b[0] && x < b[2] && y >= b[1] && y < b[3]);
        }
      }
      if (total <= cap && f.min_pixels == 1) CHECK(labelled == ink);
    }
    if (total_out) *total_out = total;
  }
  return 0;
}

static std::vector<uint8_t> noise(int w, int h, unsigned seed, unsigned per_mille) {
  std::vector<uint8_t> a((size_t)w * h);
  for (auto &v : a) {
    seed = seed * 1664525u + 1013904223u;
    v = (seed >> 8) % 1000u < per_mille ? (uint8_t)(seed >> 24) : 255;
  }
  return a;
}

int main() {
  FindOpts f;
  long total = 0;
  // degenerate sizes
  for (int w : {1, 2, 15, 16, 17, 63, 64, 65, 200})
    for (int h : {1, 2, 5, 200}) {
      if ((long)w * h > 4000) continue;
      for (int rx : {1, 16})
        for (int ry : {1, 16}) {
          f = FindOpts{};
          f.reach_x = rx; f.reach_y = ry;
          CHECK(run(std::vector<uint8_t>((size_t)w * h, 0), w, h, 0, f, 1 << 20, &total) == 0 && total == 1);    // all ink
          CHECK(run(std::vector<uint8_t>((size_t)w * h, 255), w, h, 0, f, 1 << 20, &total) == 0 && total == 0);  // blank
          CHECK(run(noise(w, h, (unsigned)(w * 131 + h), 300), w, h, 0, f, 1 << 20) == 0);
          CHECK(run(noise(w, h, (unsigned)(w * 17 + h), 300), w, h, 0, f, 1) == 0);  // cap 1
        }
    }
  // reach 16 at every border: two pixels 16 and 17 apart against each edge and corner
  for (int d : {16, 17}) {
    const int w = 40, h = 40;
    const int spots[][4] = {{0, 0, d, 0}, {0, 0, 0, d}, {0, 0, d, d}, {w - 1 - d, 0, w - 1, d}, {0, h - 1 - d, d, h - 1}, {w - 1, h - 1 - d, w - 1, h - 1},
                            {w - 1 - d, h - 1, w - 1, h - 1}, {w - 1, 0, w - 1 - d, d}, {d, h - 1 - d, 0, h - 1}};
    for (const auto &s : spots) {
      std::vector<uint8_t> a((size_t)w * h, 255);
      a[(size_t)s[1] * w + s[0]] = 0;
      a[(size_t)s[3] * w + s[2]] = 0;
      f = FindOpts{};
      f.reach_x = f.reach_y = 16;
      CHECK(run(a, w, h, 0, f, 10, &total) == 0 && total == (d == 16 ? 1 : 2));
    }
  }
  // filter, both orders, ink levels, caps around the total, on a picture with many components
  const std::vector<uint8_t> busy = noise(150, 90, 7u, 120);
  for (int order : {kOrderRaster, kOrderLeft})
    for (int min_pixels : {1, 2, 5})
      for (int level : {1, 128, 255})
        for (int cap : {1, 3, 100000}) {
          f = FindOpts{};
          f.order = order; f.min_pixels = min_pixels; f.ink_level = level; f.reach_x = 2;
          CHECK(run(busy, 150, 90, 0, f, cap) == 0);
        }
  // the most components a picture can hold: isolated pixels on every second row and column
  {
    const int w = 65, h = 33;
    std::vector<uint8_t> a((size_t)w * h, 255);
    for (int y = 0; y < h; y += 2)
      for (int x = 0; x < w; x += 2) a[(size_t)y * w + x] = 0;
    f = FindOpts{};
    CHECK(run(a, w, h, 0, f, 1 << 20, &total) == 0 && (size_t)total == max_components(w, h));
  }
  // a view with a row stride: the bytes between the rows are ink that must not be read as such
  {
    const int w = 37, h = 20, stride = 64;
    std::vector<uint8_t> a((size_t)(h - 1) * stride + w, 0);  // exactly the bytes a strided reader may touch
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) a[(size_t)y * stride + x] = (x + y) % 5 ? 255 : 0;
    f = FindOpts{};
    CHECK(run(a, w, h, stride, f, 1 << 20) == 0);
  }
  // validation
  int box[4];
  f = FindOpts{};
  CHECK(validate_find("t", 10, 10, &f, box, 1).empty());
  CHECK(!validate_find("t", 10, 10, nullptr, box, 1).empty() && !validate_find("t", 10, 10, &f, nullptr, 1).empty());
  CHECK(!validate_find("t", 10, 10, &f, box, 0).empty() && !validate_find("t", 4097, 4096, &f, box, 1).empty());
  CHECK(validate_find("t", 4096, 4096, &f, box, 1).empty());
  for (int field = 0; field < 5; field++)
    for (int bad : {-1, 0, 17, 256, 1 << 30}) {
      FindOpts g;
      int *slot[] = {&g.ink_level, &g.reach_x, &g.reach_y, &g.min_pixels, &g.order};
      *slot[field] = bad;
      const bool fine = (field == 0 && bad == 17) || (field == 3 && bad > 0) || (field == 4 && bad == 0);
      CHECK(validate_find("t", 10, 10, &g, box, 1).empty() == fine);
    }
  std::printf("components sanitize run ok\n");
  return 0;
}
