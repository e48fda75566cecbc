// runtime.hip -- host side of the MI355X runtime: device state, workspace,
// batch chunking, timing, output decode, and the C ABI of include/bnn_mi355x.h.
//
// Host-side reference code this replaces (the RAWHLS half of
// bnn/src/library/host/foldedmv-offload.{h,cpp} and rawhls-offload.cpp, plus
// the per-network bnn/src/network/<net>/sw/main_python.cpp):
//   FoldedMVInit / FoldedMVDeinit            -> Workspace (HBM buffers, lazily sized)
//   FoldedMVLoadLayerMem / DoMemInit         -> packed_params.cpp + one hipMemcpy
//   parse_cifar10 / parse_mnist_images       -> open_image_file + k_strip_records (file streamed to HBM as it lies on disk)
//   quantiseAndPack / binarizeAndPack        -> done on the GPU (k_conv0 / k_lfc_binarize)
//   BlackBoxJam(.., numReps)                 -> run_cnv / run_lfc (kernels.hip)
//   copyFromLowPrecBuffer + argmax / log2    -> k_fclast / host decode below
//
// There is no CPU compute path in this library: without a usable HIP device
// every inference entry point fails loudly (message on stderr, NULL / -1).
#include <hip/hip_runtime.h>

#include <fcntl.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include <sys/stat.h>
#include <sys/uio.h>
#include <sched.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <random>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/bnn_mi355x.h"
#include "faults.h"
#include "act_faults.h"
#include "input_faults.h"
#include "mem_faults.h"
#include "mem_org.h"
#include "kernels.h"
#include "preprocess.h"
#include "resample.h"
#include "window_kernels.h"
#include "windows.h"
#include "scan_kernels.h"
#include "scan.h"
#include "scan_clip_kernels.h"
#include "scan_clip.h"
#include "pixfmt_kernels.h"
#include "pixfmt.h"
#include "detect_kernels.h"
#include "component_kernels.h"
#include "components.h"
#include "glyph_kernels.h"
#include "glyphs.h"
#include "page.h"
#include "page_kernels.h"
#include "packed_params.h"
#include "pack_inputs.h"
#include "topology.h"

#ifndef BNN_NETWORK
#error "compile with -DBNN_NETWORK=NET_CNVW1A1 (or another bnn::NetId)"
#endif
// BNN_VARIANT: the library is built under the name of one of the fork's hardened overlays
// (cnvW1A1-TMR, ...-interleaved, ...): same compute as BNN_NETWORK, same parameter files; the fault
// entry points it shares with the base network refuse.  The hardened memory upset campaigns (mem_org.h)
// take the scheme as an argument and carry no BNN_VARIANT guard.

namespace bnn {
namespace {

constexpr int kMaxChunk = 131072;  // images per pass through the stages
constexpr int kMaxRuns = 4096;      // campaigns per bnn_mi355x_fault_campaigns call (each holds a copy of the blob in HBM)
constexpr long long kMaxSweepPairs = 16LL * kMaxChunk;  // (fault, image) pairs of one bnn_mi355x_fault_sweep run group
constexpr int kInputStagePairs = kMaxChunk;  // (run or site, image) pairs of one group of the input-fault entry points: their staged images in HBM
constexpr int kForkMin = 16384;     // images: a device-pointer pass of a CNV net of this size and more forks over the two compute lanes
constexpr int kStageSlots = 4;      // HBM staging buffers of the host paths: two on one compute lane, four on two
// Events that only TIME device work: a device-scope release at the record point instead of a flush to system scope
// ("useful to obtain more precise timings of commands between events", hip_runtime_api.h).  Nothing on the host reads
// results on the strength of these events: every entry point fetches them with a copy + stream synchronisation.
constexpr unsigned kTimeEventFlags = hipEventReleaseToDevice;
constexpr int kHostChunk = 32768;  // host-buffer / file path: H2D of chunk i+1 overlaps the stages of chunk i (largest chunk; LFC nets)
constexpr int kHostChunkCnv = 16384;  // ... the CNV nets since the chunks run on two compute lanes (below)
constexpr int kHeadChunk = 512;    // ... the first chunk: what the stages wait for before anything runs
constexpr int kFastGrowthBelow = 4096;  // ... chunks double up to here, then grow by half
// Pinned, device-mapped I/O block (ensure_io): small calls cross the PCIe link by the kernels' own loads and stores --
// no hipMemcpy, no staging, one wait.  Input area: a single CIFAR record (body 16-byte aligned) or up to kDirectMaxLfc
// host-binarised MNIST images; result area: classes / raw words of up to kMappedResMax images, scores of kMappedScoresMax.
constexpr int kDirectMaxLfc = 1024;   // images: an LFC call up to here is binarised by the calling thread and read in place
constexpr int kDirectMaxCnv = 32;     // CIFAR images from a host buffer (classify_image(s) of a few pictures: whole call 38-46 us against 46-59 through a copy,
                                      // profiles/r04_small_n_latency.txt; beyond ~64 the kernels' reads over the link cost more than the copy); from a FILE: one
constexpr int kMappedResMax = 32768, kMappedScoresMax = 256;
constexpr size_t kIoInBytes = 256u << 10;
constexpr size_t kIoClassesOff = kIoInBytes, kIoWordsOff = kIoClassesOff + (size_t)kMappedResMax * 4,
                 kIoScoresOff = kIoWordsOff + (size_t)kMappedResMax * 8, kIoDoneOff = kIoScoresOff + (size_t)kMappedScoresMax * 128,
                 kIoBytes = kIoDoneOff + 64;  // (the last 64 bytes: the completion word of single-image calls timed by the host)
static_assert((size_t)kDirectMaxLfc * kLfcWords * 8 <= kIoInBytes && 16 + 3073 <= kIoInBytes && 16 + (size_t)kDirectMaxCnv * 3072 <= kIoInBytes,
              "input area too small");

// Chunk boundaries of a host-buffer / file call: base[c] .. base[c+1] are the images of chunk c.
// The pipeline is copy | stages, double buffered per compute lane.  With equal chunks the first copy (32 768 CIFAR records
// = 100 MB: ~3 ms of pread + H2D) runs with the GPU idle, so the chunks ramp up -- by a factor that keeps the NEXT chunk's
// transfer about as long as THIS chunk's stages, or the stages starve at every step of the ramp (measured with a device
// timeline, profiles/r03_host_path_timelines.txt: doubling 2 048 -> 32 768 left 0.3-0.8 ms holes).  Both sources arrive
// faster than the stages consume them (a buffer in host memory at 54 GB/s = 17.6 M CIFAR images/s, a file through the
// pinned ring and two DMA queues at ~46 GB/s = 15 M/s, against 12.5 M/s of stages at full-size chunks), so a call is
// compute-bound: what ends it is the last chunk's stages whatever their size -- no ramp down.  Round 4, on the reference's
// own call size (a 10 000-record test-set file: 30 MB, 0.94 ms of stages): the first chunk's transfer is the one thing
// nothing hides, and small chunks run their stages at 7-10 M images/s -- half the link's rate -- so the head of the plan is
// 512 images and DOUBLES up to 4 096 (the next transfer still fits behind the current stages), then grows by half up to
// 16 384 (CNV; the LFC nets: four times these sizes in images, an MNIST image is a quarter of a CIFAR one):
// 10 000 records from a file 1.59 -> 1.25 ms, from a buffer 1.16 -> 1.14 ms on the plan alone
// (profiles/r04_small_call_plan_sweep.txt; r03_chunk_plan_sweep.txt and r03_two_lanes_plan_sweep.txt for the large calls).
// The chunks alternate over two compute lanes ("Two compute lanes" below): one chunk's launch gaps and tails are filled by
// the other's kernels.
// BNN_MI355X_CHUNKS=head:tail:max[:growth%] overrides the sizes (0 = no ramp at that end; a growth given here applies
// to every step; tuning / A-B runs).
std::vector<int> plan_chunks(int n, bool single, bool /*from_file*/) {
  // (sizes are tuned in bytes on CIFAR records: an MNIST image is a quarter of one)
  // The LFC nets' host paths ship binarised words (104 bytes per image, "binarizeAndPack on the host" below): what a chunk
  // waits for is its share of the binarising cores' work, not the link, and the one-launch kernel is at its best on large
  // chunks -- 8 192 images first, doubling (131 072 images: 102 M images/s with 2 048 first, 115-119 M with 8 192;
  // 10 000 images as ONE chunk 62 M/s against 53 M/s in three; profiles/r04_small_call_plan_sweep.txt).
  const bool cnv = net_spec(BNN_NETWORK).is_cnv;
  const int scale = cnv ? 1 : 4;
  // ... and a CNV call of 8 192 ... 32 767 images ramps DOWN as well: at that size the bytes arrive about as fast as small
  // chunks' stages consume them, and what follows the last byte is the last chunk's stages.  Interleaved A/B
  // (tools/plan_ab.py, profiles/r04_plan_ab_interleaved.txt, medians of 20-40 rounds): 10 000 images from a file 1.243 ->
  // 1.228 ms, from a buffer 1.137 -> 1.132; 20 000 images 2.297 -> 2.251 / 2.065 -> 2.059; 5 000 images LOSE 3-4 % to the two
  // extra chunks, 131 072 images 3 %: those keep the one-sided ramp.
  int head = cnv ? kHeadChunk : 8192, tail = (cnv && n >= 8192 && n < 32768) ? kHeadChunk : 0, big = cnv ? kHostChunkCnv : kHostChunk, growth = cnv ? 0 : 200;
  if (const char *e = std::getenv("BNN_MI355X_CHUNKS")) {
    int h = 0, t = 0, b = 0, g = 150;
    const int got = std::sscanf(e, "%d:%d:%d:%d", &h, &t, &b, &g);
    // (head and tail are clamped to `max`: no field of the override can ask for a chunk above the activation workspace)
    if (got >= 3 && b >= 256 && b <= kMaxChunk && h >= 0 && t >= 0 && g > 100 && g <= 400) { head = h < b ? h : b; tail = t < b ? t : b; big = b; growth = g; }
  }
  std::vector<int> front, back;
  int rem = n;
  // nothing worth overlapping: one chunk -- but never one above the largest chunk of the plan (`single`, the stage-output
  // hook, is limited to kHostChunk images by its caller)
  if ((single && n <= kMaxChunk) || (n <= 2LL * head && n <= big)) {
    front.push_back(n);
    rem = 0;
  }
  auto grow = [&](int s) {
    const int pct = growth ? growth : (s < kFastGrowthBelow * scale ? 200 : 150);
    const long long g = ((long long)s * pct / 100 + 255) & ~255LL;  // whole 256-image blocks
    return (int)(g < big ? g : big);
  };
  int sf = head > 0 ? head : big, sb = tail > 0 ? tail : big;
  if (sf > big) sf = big;
  while (rem > 0) {
    int t = sf < rem ? sf : rem;
    front.push_back(t);
    rem -= t;
    sf = grow(sf);
    if (rem > 0 && sb < big) {
      t = sb < rem ? sb : rem;
      back.push_back(t);
      rem -= t;
      sb = grow(sb);
    }
  }
  // a small remainder joins the chunk in front of it (a chunk of a few hundred images costs nine launches all the same)
  // (with a ramp at both ends the remainder is the chunk in the middle)
  if (front.size() >= 2 && front.back() * 2 < front[front.size() - 2] && front.back() + front[front.size() - 2] <= big) {
    front[front.size() - 2] += front.back();
    front.pop_back();
  }
  std::vector<int> base;
  base.push_back(0);
  for (int t : front) base.push_back(base.back() + t);
  for (size_t i = back.size(); i-- > 0;) base.push_back(base.back() + back[i]);
  return base;
}
int largest_chunk(const std::vector<int> &base) {
  int m = 0;
  for (size_t c = 0; c + 1 < base.size(); c++) m = base[c + 1] - base[c] > m ? base[c + 1] - base[c] : m;
  return m;
}

// Grow-only device buffer: the pointer and its capacity in elements are one object, so one cannot be freed without the
// other being zeroed.  Every buffer joins the registry when it is constructed: free_workspace() reaches each of them there, and a
// new buffer is one member of Runtime (the one Runtime lives as long as the library: nothing ever leaves the registry).
struct DeviceBufBase {
  void *ptr = nullptr;
  size_t cap = 0;
  static std::vector<DeviceBufBase *> &registry() {
    static std::vector<DeviceBufBase *> v;
    return v;
  }
  DeviceBufBase() { registry().push_back(this); }
  DeviceBufBase(const DeviceBufBase &) = delete;
  DeviceBufBase &operator=(const DeviceBufBase &) = delete;
  int grow_to(size_t need, size_t elem_bytes);
  void release() {
    (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
};
template <typename T>
struct DeviceBuf : DeviceBufBase {
  T *get() const { return static_cast<T *>(ptr); }
  operator T *() const { return get(); }
  // room for `need` elements (contents are not preserved)
  int grow(size_t need) { return grow_to(need, sizeof(T)); }
};

struct Runtime {
  const NetSpec &spec = net_spec(BNN_NETWORK);
  int device = -1;  // -1: whatever HIP's current device is
  std::string err;
  // parameters
  RawParams raw;  // the reference-layout memories (empty when the blob was imported)
  std::vector<uint8_t> blob;
  void *d_blob = nullptr;
  size_t d_blob_bytes = 0;
  uint64_t fault_seed = 0;  // 0: std::random_device, like the reference
  int debug_last_stage = -1;  // >= 0: stop after this stage (bnn_mi355x_debug_stage_output)
  std::vector<Fault> last_faults;
  const uint32_t *rows[9] = {};
  const uint8_t *l0_mfma = nullptr;  // layer 0 as an MFMA operand (CNV nets), unless BNN_MI355X_L0=valu
  uint8_t *d_l1_mfma = nullptr;      // cnvW1A1, BNN_MI355X_L1=mfma only: layer 1 as FP4 MFMA operands (side experiment)
  bool l1_mfma = false, l1_literal = false;  // BNN_MI355X_L1=mfma / =lds (comparison figures, never the default)
  // CNV layers 1-3 as FP4 MFMA operands (kernels.h, conv_mfma_table / conv_mfma_a2_table), made on the device from the blob's
  // rows whenever they change; null under BNN_MI355X_CONV=valu.  conv_xnor: the call in progress runs the XNOR-popcount kernels only.
  uint8_t *d_conv_mfma = nullptr;
  bool conv_mfma = false, conv_xnor = false;
  bool warmed = false;  // warm_up() has run since the last deinit()
  int two_rows = 0;  // rows holding a weight of -2 (2-bit-weight net under fault injection): kernels.hip, two_extra
  // workspace
  int cap = 0;
  void *buf0 = nullptr, *buf1 = nullptr;
  // second compute lane of the host paths ("Two compute lanes" below): its own workspace and stream
  int cap2 = 0;
  void *buf0b = nullptr, *buf1b = nullptr;
  hipStream_t stream2 = nullptr;
  hipEvent_t lane2_done = nullptr;
  hipStream_t feed_aux = nullptr;  // the pinned ring's second DMA queue (Feeder::aux), created with the streams above
  // host-buffer path: two image staging buffers in HBM (ping-pong) + results for the whole call
  int stage_cap = 0;
  // (kStageSlots buffers exist once a call has run on two lanes: each lane consumes one while the next chunk of each arrives)
  int stage_slots = 0;
  uint8_t *d_images[kStageSlots] = {};
  size_t res_cap = 0;
  int16_t *d_scores = nullptr;
  int32_t *d_classes = nullptr;
  uint64_t *d_words = nullptr;
  hipStream_t stream = nullptr, copy_stream = nullptr;
  // pinned host memory the GPU addresses directly (kIo* above): h_io as the CPU sees it, d_io as the kernels do
  uint8_t *h_io = nullptr, *d_io = nullptr;
  hipEvent_t io_t0 = nullptr, io_t1 = nullptr;  // device time of a direct call (system-scope release: the host reads what the kernels wrote)
  unsigned io_seq = 0;                           // completion marks handed out so far (BNN_MI355X_DIRECT_TIMING=host)
  std::vector<uint8_t> h_scratch;               // direct LFC calls from a file: the pixels on their way to the binariser
  // results of calls above kMappedResMax images: ONE D2H at the end of the call into pinned memory (a pageable destination
  // would be staged by the runtime), handed to the caller / decoded from there
  int32_t *h_classes = nullptr;
  uint64_t *h_words = nullptr;
  size_t h_classes_cap = 0, h_words_cap = 0;
  // The activation workspace (buf0/buf1, d_words) is shared by every call.  Host-path calls drain r.stream
  // before they return; bnn_mi355x_inference_device leaves work in flight on the CALLER's stream, so it marks
  // the end of that work with ws_event and the next call on any other stream waits for it first.
  hipEvent_t ws_event = nullptr;
  hipStream_t ws_last = nullptr;  // the caller's stream of that call (may be the null stream: hence the flag)
  bool ws_pending = false;
  // (both workspaces since such a call may fork over the two lanes: the library's own two streams each remember the last
  // hand-over they have waited for, a caller's stream waits whenever one is pending)
  uint64_t ws_gen = 0, ws_seen[2] = {0, 0};
  hipEvent_t fork_ev = nullptr;
  hipEvent_t copied[kStageSlots] = {}, consumed[kStageSlots] = {};
  std::vector<hipEvent_t> time_events;
  // file path: records as they lie on disk, two host chunks (filled by reader threads) and two HBM chunks
  size_t file_cap = 0;
  std::unique_ptr<uint8_t[]> h_file[2];
  uint8_t *d_file[2] = {nullptr, nullptr};
  hipEvent_t file_sent[2] = {nullptr, nullptr};
  DeviceBuf<uint8_t> d_all;  // a whole input file's images, resident (fault campaigns)
  // bnn_mi355x_fault_campaigns: the runs' blob copies; the staging area (patches, patch spans, segment records); results
  DeviceBuf<uint8_t> d_copies, d_camp, d_camp_res;
  std::vector<Fault> camp_faults;  // the faults of the last such call, run-major; camp_run[i]: the run of camp_faults[i]
  std::vector<int> camp_run;
  // bnn_mi355x_fault_sweep (the runs' blob copies: d_copies): the fault-free stage outputs and results of the call's images;
  // a run group's patches (staging + spans), segment records, survivor flags, results, counts + offsets, {image, class} pairs
  DeviceBuf<uint8_t> d_sw_base, d_sw_stage, d_sw_segs, d_sw_alive, d_sw_res, d_sw_cnt, d_sw_diffs;
  std::vector<long> sweep_pairs;  // the last sweep: per layer, the (fault, image) pairs it had to run (bnn_mi355x_last_sweep_stages)
  std::vector<long> act_sweep_pairs;  // the same of the last activation-fault sweep (bnn_mi355x_last_act_sweep_stages)
  // bnn_mi355x_sweep_profile: whether the single-fault sweeps record a propagation profile; a run group's [run][2]
  // counters in HBM; the last profiled sweep's [record][layer] images and activations that differ, its records and columns
  bool sweep_profile = false;
  DeviceBuf<uint8_t> d_sw_prof;
  std::vector<long> prof_alive, prof_flipped;
  long prof_rows = 0;
  int prof_cols = 0;
  // bnn_mi355x_act_noise_campaigns: run seeds and [run][layer] upset counters in HBM (segment records: d_sw_segs, results:
  // d_camp_res); the counts and seeds of the last such call
  DeviceBuf<uint8_t> d_noise;
  std::vector<long> noise_counts;
  std::vector<unsigned long long> noise_seeds;
  // bnn_mi355x_input_fault_sweep / bnn_mi355x_input_noise_campaigns: a group's faulted images; the last sweep's pairs per layer;
  // the flips per run and the seeds of the last campaign
  DeviceBuf<uint8_t> d_in_stage;
  std::vector<long> input_sweep_pairs, input_noise_counts;
  std::vector<unsigned long long> input_noise_seeds;
  // bnn_mi355x_mem_noise_campaigns (the runs' blob copies: d_copies; patches and threshold tables: d_camp; seeds and counters:
  // d_noise): the [run][layer][2] flips and the seeds of the last such call
  std::vector<long> mem_noise_counts;
  std::vector<unsigned long long> mem_noise_seeds;
  // bnn_mi355x_hardened_mem_noise_campaigns (the same buffers): [run][layer][2][2: physical, logical] and the seeds
  std::vector<long> hmem_noise_counts;
  std::vector<unsigned long long> hmem_noise_seeds;
  // bnn_mi355x_exposure_campaigns (the same buffers; the threshold state behind the tables in d_camp):
  // [run][epoch][layer][2][2: physical bits of the epoch, logical bits after it] and the seeds
  std::vector<long> xmem_counts;
  std::vector<unsigned long long> xmem_seeds;
  // bnn_mi355x_ecc_exposure_campaigns (the same buffers): [run][epoch][layer][6: the four above, then the threshold words
  // decoded with status 1 and with status 2 after the epoch] and the seeds
  std::vector<long> emem_counts;
  std::vector<unsigned long long> emem_seeds;
  // bnn_mi355x_repair_exposure_campaigns (the same buffers): [run][epoch][layer][8: the six above, then the words the
  // epoch's repair rewrote and the words of the repaired memories still unlike the loaded ones after it] and the seeds
  std::vector<long> rmem_counts;
  std::vector<unsigned long long> rmem_seeds;
  // bnn_mi355x_wecc_exposure_campaigns (the same buffers; the weight state behind the threshold state in d_camp):
  // [run][epoch][layer][12: the eight above, then the weight code words at decode status 1 and 2 after the epoch, those the
  // epoch's repair rewrote and those still unlike the loaded ones after it] and the seeds
  std::vector<long> wmem_counts;
  std::vector<unsigned long long> wmem_seeds;
  // bnn_mi355x_iwecc_exposure_campaigns (the same twelve, the code words counted after gathering) and the seeds
  std::vector<long> iwmem_counts;
  std::vector<unsigned long long> iwmem_seeds;
  // picture -> CIFAR record (bnn_mi355x_images_to_cifar): source picture, horizontal-pass output,
  // coefficient tables, records
  DeviceBuf<uint8_t> d_pp_src, d_pp_tmp, d_pp_rec;
  DeviceBuf<int32_t> d_pp_coef;
  // windows of one scene -> records / classes (bnn_mi355x_windows_to_cifar, bnn_mi355x_classify_windows): the scene, the
  // boxes + grouped order + coefficient tables (one upload), the 3072-byte bodies; upload / kernels / pass time stamps
  DeviceBuf<uint8_t> d_win_scene, d_win_body;
  DeviceBuf<int32_t> d_win_meta;
  hipEvent_t win_ev[3] = {nullptr, nullptr, nullptr};
  // the dense scan (bnn_mi355x_scan_*; scan.h): the planar picture (or a level's), the interleaved scene of scan_scene, the
  // first resize pass's output, the levels' coefficient tables (one upload), the two map buffers; time stamps around every
  // resize and every scan of a call
  DeviceBuf<uint8_t> d_scan_planes, d_scan_scene, d_scan_tmp, d_scan_buf0, d_scan_buf1;
  DeviceBuf<int32_t> d_scan_coef;
  std::vector<hipEvent_t> scan_ev;
  // the clip scan (bnn_mi355x_scan_clip*; scan_clip.h) shares the scan's buffers -- d_scan_scene holds the clip, d_scan_planes
  // every level's planes of every frame -- and adds the stage launches' lookup tables (one upload per call)
  DeviceBuf<int32_t> d_scan_clip_tab;
  // the detections (bnn_mi355x_detect_windows, bnn_mi355x_detect_clip; detect.h): the uploaded scores of detect_windows, a
  // key per window, one frame's packed boxes, and dets + counts + n_candidates of all frames; time stamps around the launches
  DeviceBuf<int16_t> d_det_scores;
  DeviceBuf<uint32_t> d_det_keys;
  DeviceBuf<uint64_t> d_det_boxes;
  DeviceBuf<int32_t> d_det_out;
  hipEvent_t det_ev[2] = {nullptr, nullptr};
  // camera frames (bnn_mi355x_unpack_frames, bnn_mi355x_*_clip_frames; pixfmt.h): the uploaded raw frames, which
  // k_unpack_frames turns into the RGB frames at d_scan_scene; time stamps around the launch of unpack_frames
  DeviceBuf<uint8_t> d_clip_raw;
  hipEvent_t pix_ev[2] = {nullptr, nullptr};
  // one picture and N boxes -> MNIST-format records / classes (bnn_mi355x_enhance_picture, bnn_mi355x_glyphs_to_mnist,
  // bnn_mi355x_classify_glyphs; LFC): the picture, its L plane, boxes + found ink boxes, descriptors + tables, the global
  // temporary of glyphs past the LDS budget, the 784-byte records, the plane's pixel sum; time stamps as win_ev
  DeviceBuf<uint8_t> d_gl_src, d_gl_plane, d_gl_tmp, d_gl_rec;
  DeviceBuf<int32_t> d_gl_box, d_gl_plan;
  DeviceBuf<unsigned long long> d_gl_sum;
  hipEvent_t gl_ev[3] = {nullptr, nullptr, nullptr};
  // the glyphs of a picture (bnn_mi355x_find_glyphs, bnn_mi355x_read_glyphs; components.h): ink words, the label plane, the
  // components by root number, head + compacted list, and -- when the label map is asked for -- the index per root number
  // and the relabelled plane; time stamps around the labelling launches and what they measured in the last call
  DeviceBuf<uint64_t> d_cc_bits;
  DeviceBuf<int32_t> d_cc_label, d_cc_list, d_cc_index, d_cc_out;
  DeviceBuf<Component> d_cc_stat;
  hipEvent_t cc_ev[2] = {nullptr, nullptr};
  float cc_usec = 0.f;
  // optional per-stage profiling (bnn_mi355x_profile): one event set per enqueued chunk
  bool profiling = false;
  std::vector<std::vector<hipEvent_t>> prof_sets;
  size_t prof_used = 0;
};

Runtime &rt() {
  static Runtime r;
  return r;
}

int fail(const std::string &msg) {
  rt().err = msg;
  std::fprintf(stderr, "bnn-mi355x[%s]: %s\n", rt().spec.name, msg.c_str());
  return -1;
}
// the refusal of every entry point that takes number_class; true: refused
bool bad_number_class(int number_class) {
  if (number_class >= 1 && number_class <= 64) return false;
  fail("number_class must be in 1..64");
  return true;
}
int launch_failed(const char *what, hipError_t e) { return fail(std::string(what) + ": kernel launch: " + hipGetErrorString(e)); }

// BNN_MI355X_TRACE=1: host-side time stamps of a host-data call (microseconds since its start) on stderr -- where a call's
// wall time goes that no device timeline shows (tools/small_call_sweep.py prints them next to the rates)
struct CallTrace {
  const bool on = std::getenv("BNN_MI355X_TRACE") != nullptr;
  std::chrono::steady_clock::time_point t0;
  std::vector<std::pair<std::string, double>> marks;
  double now() const { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
  void start() {
    if (!on) return;
    t0 = std::chrono::steady_clock::now();
    marks.clear();
  }
  void mark(const char *what, int k = -1) {
    if (!on) return;
    marks.emplace_back(k < 0 ? std::string(what) : std::string(what) + "[" + std::to_string(k) + "]", now());
  }
  void dump(const char *title) {
    if (!on) return;
    std::string line = std::string("bnn-mi355x trace ") + title + ":";
    char buf[64];
    for (auto &m : marks) {
      std::snprintf(buf, sizeof buf, " %s=%.0f", m.first.c_str(), m.second);
      line += buf;
    }
    std::fprintf(stderr, "%s\n", line.c_str());
    marks.clear();
  }
};
CallTrace &trace() {
  static CallTrace t;
  return t;
}

#define HIP_OK(expr)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

int bind_device() {
  Runtime &r = rt();
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail("no HIP device available: this runtime has no CPU fallback");
  if (r.device >= 0) HIP_OK(hipSetDevice(r.device));
  else HIP_OK(hipGetDevice(&r.device));  // first use: the calling thread's current device is this library's from now on
  if (!r.stream) {
    // Four streams in all with the feeder's second DMA queue (Feeder::aux) -- and no more: the runtime maps a process's
    // streams onto four hardware queues, a fifth stream shares one with an earlier stream and the two then serialise.
    // Found the hard way in round 4: a third compute lane (its stream created here) put Feeder::aux on this stream's
    // queue and cost the file path 20 % (131 072 records 11.3 -> 13.6 ms) before a single chunk ran on it
    // (profiles/r04_third_lane_experiment.txt).
    HIP_OK(hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking));
    HIP_OK(hipStreamCreateWithFlags(&r.copy_stream, hipStreamNonBlocking));
    HIP_OK(hipStreamCreateWithFlags(&r.stream2, hipStreamNonBlocking));
    // (the feeder's second DMA queue is created HERE, right behind the other three, although the feeder itself comes into
    // being only with the first call that needs it: streams the application creates in between would otherwise decide
    // which of this library's streams it shares a hardware queue with.  BNN_MI355X_FEEDER_STREAMS=1: one DMA queue.)
    {
      const char *es = std::getenv("BNN_MI355X_FEEDER_STREAMS");
      if (!es || std::atoi(es) == 2) HIP_OK(hipStreamCreateWithFlags(&r.feed_aux, hipStreamNonBlocking));
    }
    HIP_OK(hipEventCreateWithFlags(&r.lane2_done, hipEventDisableTiming));
    for (int i = 0; i < kStageSlots; i++) {
      HIP_OK(hipEventCreateWithFlags(&r.copied[i], hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&r.consumed[i], hipEventDisableTiming));
    }
    HIP_OK(hipEventCreateWithFlags(&r.ws_event, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&r.fork_ev, hipEventDisableTiming));
  }
  return 0;
}

// time stamps of the picture entry points, created at first use (they are not destroyed at deinit())
int ensure_events(hipEvent_t *ev, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!ev[i]) HIP_OK(hipEventCreate(&ev[i]));
  return 0;
}
int ensure_events(std::vector<hipEvent_t> &ev, size_t n) {
  if (ev.size() < n) ev.resize(n, nullptr);
  return ensure_events(ev.data(), n);
}
// *out (may be null): the device time between two events of a finished call, in microseconds per image of n
int usec_per_image(hipEvent_t a, hipEvent_t b, size_t n, float *out) {
  float ms = 0.f;
  HIP_OK(hipEventElapsedTime(&ms, a, b));
  if (out) *out = ms * 1000.f / (float)n;
  return 0;
}

// On a failing exit nothing may still be queued that reads the caller's buffers, the host chunks or the patch
// images, or that writes the caller's result arrays: the caller is free to release them as soon as it sees
// the error.  (A successful exit has waited for its streams anyway.)
void drain_feeder();  // (the pinned ring's second DMA queue, below)
struct DrainOnFailure {
  bool armed = true;
  void ok() { armed = false; }
  ~DrainOnFailure() {
    if (!armed) return;
    Runtime &r = rt();
    if (r.stream) (void)hipStreamSynchronize(r.stream);
    if (r.stream2) (void)hipStreamSynchronize(r.stream2);
    if (r.copy_stream) (void)hipStreamSynchronize(r.copy_stream);
    drain_feeder();  // DMAs still reading the pinned ring: the next job's workers would refill it under them
  }
};

// (re)make the matrix forms' operand tables from the rows in HBM, behind whatever changed them on stream s
int make_conv_tables(hipStream_t s) {
  Runtime &r = rt();
  if (!r.conv_mfma) return 0;
  const bool a2 = r.spec.id != NET_CNVW1A1;  // cnvW1A2, cnvW2A2: two planes in, two thresholds
  if (!r.d_conv_mfma) HIP_OK(hipMalloc(reinterpret_cast<void **>(&r.d_conv_mfma), a2 ? kConvMfmaA2Bytes : kConvMfmaBytes));
  HIP_OK(a2 ? conv_mfma_a2_table(r.spec.id, r.rows, r.d_conv_mfma, s) : conv_mfma_table(r.rows, r.d_conv_mfma, s));
  HIP_OK(hipStreamSynchronize(s));  // (the second compute lane reads them too)
  return 0;
}

int upload_blob() {
  Runtime &r = rt();
  if (bind_device()) return -1;
  if (r.d_blob && r.d_blob_bytes != r.blob.size()) { HIP_OK(hipFree(r.d_blob)); r.d_blob = nullptr; }
  if (!r.d_blob) {
    HIP_OK(hipMalloc(&r.d_blob, r.blob.size()));
    r.d_blob_bytes = r.blob.size();
  }
  HIP_OK(hipDeviceSynchronize());  // a reload (fault campaigns reload per run): nothing may still read the old rows
  HIP_OK(hipMemcpy(r.d_blob, r.blob.data(), r.blob.size(), hipMemcpyHostToDevice));
  r.two_rows = count_two_rows(r.spec, r.blob);
  const PackedHeader *h = reinterpret_cast<const PackedHeader *>(r.blob.data());
  for (int l = 0; l < r.spec.nlayers; l++)
    r.rows[l] = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(r.d_blob) + h->layer[l].offset);
  const char *l0 = std::getenv("BNN_MI355X_L0");
  const bool valu = l0 && std::strcmp(l0, "valu") == 0;
  r.l0_mfma = (h->l0_mfma_offset && !valu) ? static_cast<const uint8_t *>(r.d_blob) + h->l0_mfma_offset : nullptr;
  // side experiment, never the default: layer 1 of cnvW1A1 on the matrix pipe (kernels.hip, k_l1_mfma)
  const char *l1 = std::getenv("BNN_MI355X_L1");
  r.l1_mfma = r.spec.id == NET_CNVW1A1 && l1 && std::strcmp(l1, "mfma") == 0;
  r.l1_literal = r.spec.id == NET_CNVW1A1 && l1 && std::strcmp(l1, "lds") == 0;
  if (r.l1_mfma) {
    std::vector<uint8_t> tab(kL1MfmaBytes);
    l1_mfma_table(reinterpret_cast<const uint32_t *>(r.blob.data() + h->layer[1].offset), tab.data());
    if (!r.d_l1_mfma) HIP_OK(hipMalloc(reinterpret_cast<void **>(&r.d_l1_mfma), kL1MfmaBytes));
    HIP_OK(hipMemcpy(r.d_l1_mfma, tab.data(), kL1MfmaBytes, hipMemcpyHostToDevice));
  }
  const char *cv = std::getenv("BNN_MI355X_CONV");
  r.conv_mfma = r.spec.is_cnv && !(cv && std::strcmp(cv, "valu") == 0);
  return make_conv_tables(r.stream);
}

void free_workspace() {
  Runtime &r = rt();
  const auto &grown = DeviceBufBase::registry();
  if (r.cap == 0 && r.cap2 == 0 && r.stage_cap == 0 && r.res_cap == 0 && !r.file_cap && !r.h_io && !r.h_classes && !r.h_words &&
      std::none_of(grown.begin(), grown.end(), [](const DeviceBufBase *b) { return b->ptr != nullptr; }))
    return;
  if (r.device >= 0) (void)hipSetDevice(r.device);
  (void)hipDeviceSynchronize();
  if (r.h_io) (void)hipHostFree(r.h_io);
  r.h_io = r.d_io = nullptr;
  if (r.h_classes) (void)hipHostFree(r.h_classes);
  if (r.h_words) (void)hipHostFree(r.h_words);
  r.h_classes = nullptr; r.h_words = nullptr;
  r.h_classes_cap = r.h_words_cap = 0;
  r.h_scratch = std::vector<uint8_t>();
  (void)hipFree(r.buf0); (void)hipFree(r.buf1);
  for (auto &b : r.d_images) { (void)hipFree(b); b = nullptr; }
  (void)hipFree(r.d_scores); (void)hipFree(r.d_classes); (void)hipFree(r.d_words);
  r.buf0 = r.buf1 = nullptr;
  r.d_scores = nullptr; r.d_classes = nullptr; r.d_words = nullptr;
  r.cap = r.stage_cap = r.stage_slots = 0;
  r.res_cap = 0;
  (void)hipFree(r.buf0b); (void)hipFree(r.buf1b);
  r.buf0b = r.buf1b = nullptr;
  r.cap2 = 0;
  (void)hipFree(r.d_file[0]); (void)hipFree(r.d_file[1]);
  r.d_file[0] = r.d_file[1] = nullptr;
  r.h_file[0].reset(); r.h_file[1].reset();
  r.file_cap = 0;
  for (DeviceBufBase *b : grown) b->release();
}

int DeviceBufBase::grow_to(size_t need, size_t elem_bytes) {
  if (need <= cap) return 0;
  HIP_OK(hipStreamSynchronize(rt().stream));
  release();
  const size_t n = need + need / 4 + 256;
  HIP_OK(hipMalloc(&ptr, n * elem_bytes));
  cap = n;
  return 0;
}

// grow-only pinned host buffer (contents are not preserved)
template <typename T>
int grow_pinned(T *&ptr, size_t &cap, size_t need) {
  if (need <= cap) return 0;
  if (ptr) {
    HIP_OK(hipStreamSynchronize(rt().stream));
    (void)hipHostFree(ptr);
  }
  ptr = nullptr;
  cap = 0;
  const size_t n = need + need / 4 + 256;
  HIP_OK(hipHostMalloc(reinterpret_cast<void **>(&ptr), n * sizeof(T), hipHostMallocDefault));
  cap = n;
  return 0;
}

// activation workspace for `n` images per pass (at most kMaxChunk)
int reserve(int n) {
  Runtime &r = rt();
  if (n > kMaxChunk) n = kMaxChunk;
  if (n <= r.cap) return 0;
  if (bind_device()) return -1;
  HIP_OK(hipDeviceSynchronize());
  (void)hipFree(r.buf0); (void)hipFree(r.buf1);
  r.buf0 = r.buf1 = nullptr;
  r.cap = 0;
  size_t b0, b1;
  if (r.spec.is_cnv) cnv_workspace_bytes(r.spec.abits, &b0, &b1);
  else lfc_workspace_bytes(r.spec.abits, &b0, &b1);
  HIP_OK(hipMalloc(&r.buf0, (size_t)n * b0 + 256));
  HIP_OK(hipMalloc(&r.buf1, (size_t)n * b1 + 256));
  r.cap = n;
  return 0;
}

// Two compute lanes.  A host-path call cuts its batch into chunks so that copies and kernels overlap (plan_chunks); on ONE
// stream the nine launches of every chunk follow each other with the dispatcher's gap between them and each with its
// own tail, and the small chunks at the head of the plan pay that at 2 048-8 192 images a time: the plan of 131 072
// CIFAR images takes 11.12 ms of kernels against 10.40 ms for the batch in one pass.  With the chunks alternating over
// two streams -- a second activation workspace, the staging buffer of slot s feeds lane s -- one lane's gaps and tails
// are filled by the other's kernels: 10.61 ms (tools/two_lane_probe.py, profiles/r03_two_lane_probe.txt).
// Each lane needs its own pair of staging buffers (slots_for: four in all): with two, both are held by the two chunks
// in flight, the next copy cannot start before one of them ends, and a call from a host buffer got SLOWER (1 048 576
// images 87.7 -> 100.7 ms); with four: 131 072 images from a host buffer 11.55 -> 11.3 ms, from a file 12.6-13.3 ->
// 11.7-12.0 ms, 524 288 from a file 46.1-48.3 -> 44.6-44.9 ms (profiles/r03_two_lanes_ab.txt).
// BNN_MI355X_LANES=1 forces one lane (A/B); stage profiling and the stage-output hook always run on one lane.
int lanes_for(int nchunks) {
  static const bool one = [] { const char *e = std::getenv("BNN_MI355X_LANES"); return e && std::atoi(e) == 1; }();
  const Runtime &r = rt();
  return (nchunks >= 3 && !one && !r.profiling && r.debug_last_stage < 0) ? 2 : 1;
}
// the second lane's activation workspace for `n` images per pass
int reserve2(int n) {
  Runtime &r = rt();
  if (n > kMaxChunk) n = kMaxChunk;
  if (n <= r.cap2) return 0;
  if (bind_device()) return -1;
  HIP_OK(hipDeviceSynchronize());
  (void)hipFree(r.buf0b); (void)hipFree(r.buf1b);
  r.buf0b = r.buf1b = nullptr;
  r.cap2 = 0;
  size_t b0, b1;
  if (r.spec.is_cnv) cnv_workspace_bytes(r.spec.abits, &b0, &b1);
  else lfc_workspace_bytes(r.spec.abits, &b0, &b1);
  HIP_OK(hipMalloc(&r.buf0b, (size_t)n * b0 + 256));
  HIP_OK(hipMalloc(&r.buf1b, (size_t)n * b1 + 256));
  r.cap2 = n;
  return 0;
}
// HBM staging buffers of a call on `lanes` lanes: chunk c lands in slot c % slots and runs on lane c & 1 -- with two
// buffers both would be held by the two chunks in flight and the next copy could not start before one of them ends
int slots_for(int lanes) { return lanes == 2 ? kStageSlots : 2; }
// chunk c of a call that runs on `lanes` lanes: its stream
hipStream_t lane_stream(int c, int lanes) { return (lanes == 2 && (c & 1)) ? rt().stream2 : rt().stream; }
// all chunks are enqueued: whatever follows on r.stream (the results' way back) comes behind the second lane too
int join_lanes(int lanes) {
  Runtime &r = rt();
  if (lanes == 2) {
    HIP_OK(hipEventRecord(r.lane2_done, r.stream2));
    HIP_OK(hipStreamWaitEvent(r.stream, r.lane2_done, 0));
  }
  return 0;
}
// device time of a call's chunks, ms: the union of their [t0, t1] intervals (on one lane they do not overlap: the sum)
int chunks_device_ms(int nchunks, double *out) {
  Runtime &r = rt();
  std::vector<std::pair<float, float>> iv((size_t)nchunks);
  for (int c = 0; c < nchunks; c++) {
    float a = 0.f, d = 0.f;
    if (c) HIP_OK(hipEventElapsedTime(&a, r.time_events[0], r.time_events[2 * c]));
    HIP_OK(hipEventElapsedTime(&d, r.time_events[2 * c], r.time_events[2 * c + 1]));
    iv[(size_t)c] = {a, a + d};
  }
  if (trace().on) {  // when each chunk's stages ran on the device, microseconds from the first chunk's start
    std::string line = "bnn-mi355x trace device intervals of the chunks (start-end us):";
    char buf[48];
    for (auto &x : iv) {
      std::snprintf(buf, sizeof buf, " %.0f-%.0f", x.first * 1e3, x.second * 1e3);
      line += buf;
    }
    std::fprintf(stderr, "%s\n", line.c_str());
  }
  std::sort(iv.begin(), iv.end());
  double total = 0.0;
  float lo = iv[0].first, hi = iv[0].second;
  for (int c = 1; c < nchunks; c++) {
    if (iv[(size_t)c].first > hi) { total += hi - lo; lo = iv[(size_t)c].first; hi = iv[(size_t)c].second; }
    else if (iv[(size_t)c].second > hi) hi = iv[(size_t)c].second;
  }
  *out = total + (hi - lo);
  return 0;
}

// host-buffer path: staging for `chunk` images x `slots` and result buffers for `n_total` images
int reserve_host(int chunk, size_t n_total, int slots = 2) {
  Runtime &r = rt();
  if (bind_device()) return -1;
  if (chunk > r.stage_cap || slots > r.stage_slots) {
    HIP_OK(hipDeviceSynchronize());
    if (chunk < r.stage_cap) chunk = r.stage_cap;
    if (slots < r.stage_slots) slots = r.stage_slots;
    for (auto &b : r.d_images) {
      (void)hipFree(b);
      b = nullptr;
    }
    r.stage_cap = r.stage_slots = 0;
    for (int i = 0; i < slots; i++)
      HIP_OK(hipMalloc(reinterpret_cast<void **>(&r.d_images[i]), (size_t)chunk * r.spec.image_bytes() + 256));
    r.stage_cap = chunk;
    r.stage_slots = slots;
  }
  if (n_total > r.res_cap) {
    HIP_OK(hipDeviceSynchronize());
    (void)hipFree(r.d_scores); (void)hipFree(r.d_classes); (void)hipFree(r.d_words);
    r.d_scores = nullptr; r.d_classes = nullptr; r.d_words = nullptr;
    r.res_cap = 0;
    const size_t N = n_total < 1024 ? 1024 : n_total;
    if (r.spec.is_cnv) HIP_OK(hipMalloc(reinterpret_cast<void **>(&r.d_scores), N * 64 * sizeof(int16_t)));
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&r.d_classes), N * sizeof(int32_t)));
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&r.d_words), N * sizeof(uint64_t)));
    r.res_cap = N;
  }
  return 0;
}

// the pinned, device-mapped I/O block (kIo*); once per load (warm_up) or at first use
int ensure_io() {
  Runtime &r = rt();
  if (r.h_io) return 0;
  if (bind_device()) return -1;
  void *h = nullptr, *d = nullptr;
  HIP_OK(hipHostMalloc(&h, kIoBytes, hipHostMallocMapped));
  if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess || !d) {
    (void)hipHostFree(h);
    return fail("pinned I/O block: no device address for host memory");
  }
  std::memset(h, 0, kIoBytes);
  r.h_io = static_cast<uint8_t *>(h);
  r.d_io = static_cast<uint8_t *>(d);
  if (!r.io_t0) {
    HIP_OK(hipEventCreate(&r.io_t0));
    HIP_OK(hipEventCreate(&r.io_t1));
  }
  return 0;
}

// mapped result slots of a call of n images (null: that result goes through HBM and a copy)
struct ResultSlots {
  int32_t *h_classes = nullptr, *d_classes = nullptr;
  uint64_t *h_words = nullptr, *d_words = nullptr;
  int16_t *h_scores = nullptr, *d_scores = nullptr;
};
ResultSlots mapped_results(int n, bool scores, bool direct = false) {
  Runtime &r = rt();
  ResultSlots m;
  static const bool off = std::getenv("BNN_MI355X_NO_MAPPED_RESULTS") != nullptr;  // A/B of the chunked calls (a direct call has no other way)
  if ((off && !direct) || n > kMappedResMax || (scores && n > kMappedScoresMax) || ensure_io()) return m;
  m.h_classes = reinterpret_cast<int32_t *>(r.h_io + kIoClassesOff);
  m.d_classes = reinterpret_cast<int32_t *>(r.d_io + kIoClassesOff);
  m.h_words = reinterpret_cast<uint64_t *>(r.h_io + kIoWordsOff);
  m.d_words = reinterpret_cast<uint64_t *>(r.d_io + kIoWordsOff);
  if (scores) {
    m.h_scores = reinterpret_cast<int16_t *>(r.h_io + kIoScoresOff);
    m.d_scores = reinterpret_cast<int16_t *>(r.d_io + kIoScoresOff);
  }
  return m;
}

// An earlier device-pointer call on another stream may still own the activation workspaces: work about to be queued on
// `s` waits for its end first.
int settle_handover(hipStream_t s) {
  Runtime &r = rt();
  const int own = s == r.stream ? 0 : (s == r.stream2 ? 1 : -1);
  if (own >= 0 ? (r.ws_seen[own] == r.ws_gen || r.ws_last == s) : (!r.ws_pending || r.ws_last == s)) return 0;
  {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
    // A capturing stream must not wait on an event recorded outside its capture (the capture would be invalidated, or
    // the dependency silently dropped on replay): settle the hand-over on the host before anything is recorded.
    if (cap != hipStreamCaptureStatusNone) {
      // (a host-side wait is "unsafe" under the global capture mode frameworks use: switch this thread to the relaxed
      // mode around it -- the wait is on work submitted before the capture began, which is exactly the safe case)
      hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
      HIP_OK(hipThreadExchangeStreamCaptureMode(&mode));
      const hipError_t we = hipEventSynchronize(r.ws_event);
      (void)hipThreadExchangeStreamCaptureMode(&mode);
      if (we != hipSuccess)
        return fail("inference_device: an earlier call on another stream still owns the workspace and cannot be waited for during "
                    "stream capture; synchronise that stream before capturing");
    } else {
      HIP_OK(hipStreamWaitEvent(s, r.ws_event, 0));
    }
  }
  if (own >= 0) r.ws_seen[own] = r.ws_gen;
  else r.ws_pending = false;
  return 0;
}

// enqueue one chunk (n <= cap) whose images are already in HBM
// t0 / t1 (optional): this chunk's device time is t0 -> t1 (kernels.h)
// the kernel forms a CNV batch may take with the parameters and switches now in force (run_cnv picks among them by size)
void set_forms(CnvLaunch &a) {
  Runtime &r = rt();
  a.l0_mfma = r.l0_mfma;
  a.l1_mfma = r.l1_mfma ? r.d_l1_mfma : nullptr;
  a.l1_literal = r.l1_literal;
  a.conv_mfma = r.conv_mfma && !r.conv_xnor ? r.d_conv_mfma : nullptr;
  a.has_two = r.two_rows > 0;
}

int enqueue(const uint8_t *d_imgs, int n, int ncls, int32_t *d_classes, int16_t *d_scores, uint64_t *d_words,
            hipStream_t s, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr, int lane = 0, bool t_dispatch = false, bool packed = false,
            unsigned *done_flag = nullptr, unsigned done_seq = 0) {
  Runtime &r = rt();
  hipError_t e;
  hipEvent_t *evs = nullptr;
  void *const ws0 = lane ? r.buf0b : r.buf0, *const ws1 = lane ? r.buf1b : r.buf1;
  // (the stages index the workspace by image: a chunk above its capacity would write past it on the device)
  if (n > (lane ? r.cap2 : r.cap)) return fail("internal: a chunk of " + std::to_string(n) + " images exceeds the activation workspace");
  if (settle_handover(s)) return -1;
  if (r.profiling) {
    const int need = (r.spec.is_cnv ? kCnvStages : kLfcStages) + 1;
    if (r.prof_used == r.prof_sets.size()) {
      std::vector<hipEvent_t> set(need);
      for (auto &ev : set) HIP_OK(hipEventCreate(&ev));
      r.prof_sets.push_back(set);
    }
    evs = r.prof_sets[r.prof_used++].data();
  }
  if (r.spec.is_cnv) {
    CnvLaunch a{};
    a.images = d_imgs; a.n = n; a.buf0 = ws0; a.buf1 = ws1;
    for (int l = 0; l < 9; l++) a.rows[l] = r.rows[l];
    set_forms(a);
    a.scores = d_scores; a.classes = d_classes; a.number_class = ncls; a.stream = s; a.events = evs;
    a.last_stage = r.debug_last_stage >= 0 ? r.debug_last_stage : kCnvStages - 1;
    a.t0 = t0; a.t1 = t1; a.done_flag = done_flag; a.done_seq = done_seq;
    e = run_cnv(r.spec.id, a);
  } else {
    LfcLaunch a{};
    a.images = d_imgs; a.packed = packed; a.n = n; a.buf0 = ws0; a.buf1 = ws1;
    for (int l = 0; l < 4; l++) a.rows[l] = r.rows[l];
    a.words = d_words;
    a.classes = d_classes; a.number_class = ncls; a.stream = s; a.events = evs;
    a.last_stage = r.debug_last_stage >= 0 ? r.debug_last_stage : kLfcStages - 1;
    a.t0 = t0; a.t1 = t1; a.t_dispatch = t_dispatch; a.done_flag = done_flag; a.done_seq = done_seq;
    e = run_lfc(r.spec.id, a);
  }
  if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
  return 0;
}

bool ready() {
  if (!rt().d_blob) { fail("load_parameters has not been called (or failed)"); return false; }
  return true;
}

// ---- host data -> HBM through a ring of pinned pieces --------------------------------------------------
// hipMemcpyAsync from PAGEABLE memory is a single-threaded copy into the runtime's own pinned staging plus the DMA
// (measured: 34 GB/s, 11.8 ms for 131 072 CIFAR images -- more than the 10.7 ms their stages take), and a file read
// with pread() into a pageable chunk first pays a second CPU copy (27 GB/s with 8 reader threads).  For calls of
// kFeederMinBytes and more, worker threads fill 4 MB pinned pieces -- memcpy from the caller's buffer, or pread()
// straight from the page cache -- and the calling thread, the only one that talks to HIP, sends each piece with an
// asynchronous DMA as soon as it is full: one CPU copy per byte, spread over the cores this process may use.
constexpr size_t kFeederMinBytes = 2u << 20;  // (24 MB until round 4: with the small first pieces and the caller's own first piece a 5 000-record file takes 0.80 ms through the ring, 1.03 ms through a pageable chunk)
int usable_cpus() {
  int n = 0;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
  if (n <= 0) n = (int)std::thread::hardware_concurrency();
  if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // a container's CPU quota
    long long quota = 0, period = 0;
    char q[32] = {0};
    if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0 && period > 0) {
      quota = std::atoll(q);
      const int lim = (int)(quota / period);
      if (lim >= 1 && lim < n) n = lim;
    }
    std::fclose(f);
  }
  return n > 0 ? n : 1;
}

#if defined(__x86_64__)
// write the lines of [p, p + n) back to memory and drop them from the caches (clflushopt: unordered, one fence at the end)
__attribute__((target("clflushopt"))) void flush_lines(const uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; i += 64) _mm_clflushopt(const_cast<uint8_t *>(p) + i);
  _mm_sfence();
}
#endif

struct Feeder {
  static constexpr int kSlots = 12;
  static constexpr int kMaxWorkers = 14;
  size_t kSlotBytes = 4u << 20;  // BNN_MI355X_FEEDER_PIECE_MB overrides (tuning): alone, 4 MB pieces move at 49 GB/s, 8 MB at 52, 16 MB at 54
                                 // (profiles/r03_h2d_probe.txt); behind the readers 2-4 MB pieces gave the shortest calls
  // A PIECE is what one worker fills in one go (256-512 KB of source: a pread of that size takes 20-40 us, so the pieces of
  // a group are read side by side); a GROUP is what goes to HBM with one DMA: the pieces that share ring slot
  // (group % kSlots), up to kSlotBytes -- DMAs of 1-4 MB move at the link's rate, smaller ones cost ~10 us each whatever
  // their size (round 4's first form had piece = DMA: 4 MB pieces took one reader 0.3 ms each and the last bytes of a
  // 30 MB file arrived at 1.16 ms, 256 KB pieces moved at a third of the link's rate;
  // profiles/r04_timeline_cnvW1A1_10000_file_*.txt).  RAW job (CNV records, images as they are): source bytes are copied.
  // PACKED job (LFC: binarizeAndPack on the host, csrc/pack_inputs.h): `bytes` = whole 784-byte images, their 13-word
  // forms are what lands in the ring, and a chunk is one group (104 bytes per image: 32 768 images are 3.4 MB).
  struct Piece {
    int chunk, group;
    size_t ring_off;   // where in the group's ring slot this piece's output goes
    size_t src_off;    // of its first item (record / image) in the source
    size_t items;
    bool last_of_group, last_of_chunk;
    size_t group_dst_off, group_bytes;  // (on the last piece of a group) the group's place in the chunk's HBM buffer and its size
  };
  // the items of the job in flight: `rec` source bytes each, of which the first `skip` are dropped (the label byte of a
  // CIFAR-10 record: the readers scatter the records with preadv() so that only the image bodies land in the ring -- no
  // label bytes cross the link and no kernel has to remove them)
  size_t rec = 0, skip = 0;
  uint8_t *ring = nullptr;  // kSlots x kSlotBytes, pinned
  bool ready = false;       // init() went through: ring, events, streams and workers exist
  hipEvent_t sent[kSlots] = {};
  // Two things make the pipe faster than "pread, then one DMA queue" (tools/file_pipe_probe.cpp, profiles/r03_file_pipe_probe.txt:
  // 33-37 GB/s): the pieces alternate over TWO streams, i.e. two DMA queues (46 GB/s), and the readers write their lines
  // back behind the pread (clflushopt: a DMA that finds the lines dirty in a core's cache runs at two thirds of its rate;
  // 43 GB/s on one queue).  BNN_MI355X_FEEDER_STREAMS / BNN_MI355X_FEEDER_FLUSH override.
  hipStream_t aux = nullptr;
  hipEvent_t aux_done = nullptr;
  bool flush = false;
  std::vector<std::thread> workers;
  int raw_workers = 1;  // a RAW job keeps the first raw_workers threads busy (more readers slow the DMA down), a PACKED job all of them
  std::mutex mu;
  std::condition_variable cv_job, cv_done;
  bool quit = false;
  uint64_t job_id = 0;
  // the job in flight
  const std::vector<Piece> *pieces = nullptr;
  const uint8_t *mem = nullptr;  // source: host memory ...
  int fd = -1;                   // ... or a file
  bool packed = false;
  int job_workers = 0;
  std::atomic<size_t> next{0}, released{0};  // released: groups whose DMA is done (their ring slot may be refilled)
  std::unique_ptr<std::atomic<uint8_t>[]> filled;  // per piece: 0 not yet, 1 filled, 2 failed
  size_t filled_cap = 0;
  std::atomic<bool> abort{false};
  int active = 0;  // workers that have not yet left the current job (under mu)
  // BNN_MI355X_TRACE: per worker, microseconds from begin() to its first claim, microseconds spent filling, pieces filled
  struct Stat { double first = -1, busy = 0; int pieces = 0; };
  Stat stats[kMaxWorkers + 1];
  std::chrono::steady_clock::time_point job_t0;

  uint8_t *ring_at(const Piece &pc) const { return ring + (size_t)(pc.group % kSlots) * kSlotBytes + pc.ring_off; }
  bool read_all(uint8_t *dst, size_t bytes, size_t off) const {
    size_t done = 0;
    while (done < bytes) {
      const ssize_t got = ::pread(fd, dst + done, bytes - done, (off_t)(off + done));
      if (got <= 0) return false;
      done += (size_t)got;
    }
    return true;
  }
  bool fill(const Piece &pc, uint8_t *dst) const {
    if (packed) {
      if (mem) { binarize_pack(mem + pc.src_off, pc.items, reinterpret_cast<uint64_t *>(dst)); return true; }
      // from a file: the pixels pass through a cache-sized scratch block on their way to the binariser
      constexpr size_t kBlock = 80;  // images: 62 720 bytes
      uint8_t scratch[kBlock * kLfcPixels];
      for (size_t i = 0; i < pc.items; i += kBlock) {
        const size_t m = pc.items - i < kBlock ? pc.items - i : kBlock;
        if (!read_all(scratch, m * kLfcPixels, pc.src_off + i * kLfcPixels)) return false;
        binarize_pack(scratch, m, reinterpret_cast<uint64_t *>(dst) + i * kLfcWords);
      }
      return true;
    }
    const size_t body = rec - skip;
    if (skip == 0) {
      if (mem) { std::memcpy(dst, mem + pc.src_off, pc.items * rec); return true; }
      if (!read_all(dst, pc.items * rec, pc.src_off)) return false;
    } else if (mem) {
      for (size_t i = 0; i < pc.items; i++) std::memcpy(dst + i * body, mem + pc.src_off + i * rec + skip, body);
      return true;
    } else {
      // label bytes into a bin, bodies side by side: two iovecs per record, IOV_MAX (1024) per call
      constexpr size_t kBatch = 512;
      static_assert(2 * kBatch <= 1024, "IOV_MAX");
      struct iovec iov[2 * kBatch];
      uint8_t bin[64];
      if (skip > sizeof bin) return false;
      for (size_t i = 0; i < pc.items; i += kBatch) {
        const size_t m = pc.items - i < kBatch ? pc.items - i : kBatch;
        for (size_t k = 0; k < m; k++) {
          iov[2 * k] = {bin, skip};
          iov[2 * k + 1] = {dst + (i + k) * body, body};
        }
        size_t want = m * rec, done = 0;
        off_t off = (off_t)(pc.src_off + i * rec);
        int first_iov = 0;
        while (done < want) {
          const ssize_t got = ::preadv(fd, iov + first_iov, (int)(2 * m) - first_iov, off + (off_t)done);
          if (got <= 0) return false;
          done += (size_t)got;
          if (done < want) {  // a short read: step over the iovecs that are full, trim the one that is not
            size_t g = (size_t)got;
            while (g >= iov[first_iov].iov_len) g -= iov[first_iov++].iov_len;
            iov[first_iov].iov_base = static_cast<uint8_t *>(iov[first_iov].iov_base) + g;
            iov[first_iov].iov_len -= g;
          }
        }
      }
    }
#if defined(__x86_64__)
    if (flush) flush_lines(dst, pc.items * body);
#endif
    return true;
  }
  // claim the next piece and fill it; false when none is left.  (Also called once by the thread that started the job:
  // the workers need some tens of microseconds to wake up, and the first piece is what everything waits for.)
  bool work_one(int who = kMaxWorkers) {
    const size_t np = pieces->size();
    const size_t p = next.fetch_add(1, std::memory_order_relaxed);
    if (p >= np) return false;
    const Piece &pc = (*pieces)[p];
    // (its ring slot is free once the DMA of the group that had it before is done: `released` counts finished DMAs)
    while (!abort.load(std::memory_order_relaxed) && (size_t)pc.group >= released.load(std::memory_order_acquire) + kSlots) std::this_thread::yield();
    const bool tr = trace().on;
    std::chrono::steady_clock::time_point a;
    if (tr) {
      a = std::chrono::steady_clock::now();
      if (stats[who].first < 0) stats[who].first = std::chrono::duration<double, std::micro>(a - job_t0).count();
    }
    const bool ok = !abort.load(std::memory_order_relaxed) && fill(pc, ring_at(pc));
    if (tr) {
      stats[who].busy += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count();
      stats[who].pieces++;
    }
    filled[p].store(ok ? 1 : 2, std::memory_order_release);
    return true;
  }
  void worker(int index) {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_job.wait(lk, [&] { return quit || job_id != seen; });
        if (quit) return;
        seen = job_id;
        if (index >= job_workers) continue;  // not needed for this job (and not counted in `active`)
      }
      while (work_one(index)) {}
      std::lock_guard<std::mutex> lk(mu);
      if (--active == 0) cv_done.notify_all();
    }
  }
  // pinned ring, events and worker threads: once per process (the threads sleep between jobs)
  int init() {
    if (ready) return 0;
    if (ring) return -1;  // an earlier attempt got the ring but not its events or streams: stays refused (the caller reports it)
    if (const char *e = std::getenv("BNN_MI355X_FEEDER_PIECE_MB")) {
      const int mb = std::atoi(e);
      if (mb >= 1 && mb <= 32) kSlotBytes = (size_t)mb << 20;
    }
    if (hipHostMalloc(reinterpret_cast<void **>(&ring), kSlots * kSlotBytes, hipHostMallocDefault) != hipSuccess) { ring = nullptr; return -1; }
    for (auto &e : sent)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return -1;
    const char *ef = std::getenv("BNN_MI355X_FEEDER_FLUSH");
    aux = rt().feed_aux;  // (created in bind_device, next to the library's other streams: see there)
    if (aux && hipEventCreateWithFlags(&aux_done, hipEventDisableTiming) != hipSuccess) return -1;
#if defined(__x86_64__)
    flush = (ef ? std::atoi(ef) != 0 : false) && __builtin_cpu_supports("clflushopt");
#endif
    // Readers of a RAW job: 4 pread() threads already move 45 GB/s out of the page cache (8: 74 GB/s), more than the link
    // takes; beyond ~6 the DMA, which reads the lines they have just written, slows down more than they speed up
    // (profiles/r03_file_path_sweep.txt: 2 threads 20.4 ms per 131 072-record file, 4: 12.9-14.7, 6: 14.1, 14: 14.2).
    // A PACKED job is the other way round -- 7.5 source bytes per byte that crosses the link, the binarising cores are the
    // bound -- and takes every core this process may use but two (one for the calling thread, one for the driver's).
    const int avail = usable_cpus() - 2;
    int nr = avail > 6 ? 6 : avail, nt = avail > kMaxWorkers ? kMaxWorkers : avail;
    if (const char *e = std::getenv("BNN_MI355X_FEEDER_THREADS")) nr = std::atoi(e);
    if (const char *e = std::getenv("BNN_MI355X_PACK_THREADS")) nt = std::atoi(e);
    nr = nr < 1 ? 1 : (nr > kMaxWorkers ? kMaxWorkers : nr);
    nt = nt < nr ? nr : (nt > kMaxWorkers ? kMaxWorkers : nt);
    raw_workers = nr;
    for (int i = 0; i < nt; i++) workers.emplace_back([this, i] { worker(i); });
    ready = true;
    return 0;
  }
  void begin(const std::vector<Piece> &pcs, const uint8_t *m, int f, bool pack, size_t item_bytes, size_t drop) {
    if (pcs.size() > filled_cap) {
      filled.reset(new std::atomic<uint8_t>[pcs.size()]);
      filled_cap = pcs.size();
    }
    for (size_t i = 0; i < pcs.size(); i++) filled[i].store(0, std::memory_order_relaxed);
    next = 0; released = 0; abort = false;
    if (trace().on) {
      for (auto &st : stats) st = Stat{};
      job_t0 = std::chrono::steady_clock::now();
    }
    {
      std::lock_guard<std::mutex> lk(mu);
      pieces = &pcs; mem = m; fd = f; packed = pack; rec = item_bytes; skip = drop;
      const int want = pack ? (int)workers.size() : raw_workers;
      // (no more threads than pieces: a thread woken for nothing still has to be waited for at the end)
      job_workers = (size_t)want < pcs.size() ? want : (int)pcs.size();
      active = job_workers;
      job_id++;
      cv_job.notify_all();
    }
    (void)work_one();  // the first piece by this thread, while the workers wake up
  }
  // every worker has left the job: its description may go out of scope
  void end() {
    abort = true;  // (a no-op after a complete run: nothing is left to claim)
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return active == 0; });
    if (trace().on) {
      std::string line = "bnn-mi355x trace feeder (worker: first claim us / busy us / pieces; last = the calling thread):";
      char buf[64];
      for (int i = 0; i <= kMaxWorkers; i++) {
        if (stats[i].pieces == 0) continue;
        std::snprintf(buf, sizeof buf, " %d:%.0f/%.0f/%d", i, stats[i].first, stats[i].busy, stats[i].pieces);
        line += buf;
      }
      std::fprintf(stderr, "%s\n", line.c_str());
    }
  }
};
// One per process, never destroyed: its threads sleep on a condition variable between jobs and end with the process
// (a static object's destructor would have to join them at exit, behind the HIP runtime's own teardown).
Feeder &feeder() {
  static Feeder *f = new Feeder;
  return *f;
}
void drain_feeder() {
  Feeder &f = feeder();
  if (f.aux) (void)hipStreamSynchronize(f.aux);
}
// calls of this many source bytes and more go through the ring (BNN_MI355X_FEEDER_MIN_MB overrides; tuning)
bool use_feeder(size_t bytes) {
  static const bool off = std::getenv("BNN_MI355X_NO_FEEDER") != nullptr;
  static const size_t min_bytes = [] {
    const char *e = std::getenv("BNN_MI355X_FEEDER_MIN_MB");
    return e ? (size_t)std::atoi(e) << 20 : kFeederMinBytes;
  }();
  return !off && bytes >= min_bytes;
}

// n images from host memory (fd < 0) or from an open file, cut by `plan`, through the pinned ring into the HBM chunk
// buffers; consume(c, base, m, slot) enqueues chunk c's stages on its lane's stream (lane_stream) once its bytes
// (RAW: the image bodies, the readers having dropped the `skip` label bytes of every record; PACKED: 13 words per image)
// are in r.d_images[slot] and that stream has been made to wait for them.
template <typename Consume>
int feed_chunks(const uint8_t *mem, int fd, size_t first, size_t rec, size_t skip, const std::vector<int> &plan, int lanes, bool packed, Consume consume) {
  Runtime &r = rt();
  Feeder &F = feeder();
  if (F.init()) return fail("pinned staging ring: allocation failed");
  const int nchunks = (int)plan.size() - 1, nslots = slots_for(lanes);
  if (packed && (skip || rec != (size_t)kLfcPixels || (size_t)largest_chunk(plan) * kLfcWords * 8 > F.kSlotBytes))
    return fail("internal: packed feed of a chunk that does not fit a ring slot");
  // Groups (DMAs) start small and double -- the first one is what everything else waits for --, the pieces inside them are
  // small throughout; the first chunk is one group in the smallest pieces, so that all workers share it.
  std::vector<Feeder::Piece> pieces;
  const size_t out = packed ? (size_t)kLfcWords * 8 : rec - skip;          // ring / HBM bytes per item
  const size_t piece0 = packed ? 256 : (256u << 10) / rec, piece1 = packed ? 1024 : (512u << 10) / rec;  // items per piece
  const size_t group_max = F.kSlotBytes / out;                              // items per group at most
  size_t group_want = (1u << 20) / out;                                     // RAW: 1, 2, 4 MB ...; PACKED: a chunk is a group
  int ngroups = 0;
  for (int c = 0; c < nchunks; c++) {
    const size_t items = (size_t)(plan[c + 1] - plan[c]), src0 = first + (size_t)plan[c] * rec;
    for (size_t g0 = 0; g0 < items;) {
      size_t gi = items - g0;
      if (!packed) {
        const size_t cap = c == 0 ? group_max : group_want;
        if (gi > cap) gi = cap;
        if (items - g0 - gi < gi / 4 && items - g0 <= group_max) gi = items - g0;  // (no crumb of a group at the end of a chunk)
        if (c > 0) group_want = group_want * 2 < group_max ? group_want * 2 : group_max;
      }
      const size_t psz = c == 0 ? piece0 : piece1;
      for (size_t o = 0; o < gi;) {
        const size_t b = gi - o < psz ? gi - o : psz;
        Feeder::Piece pc{};
        pc.chunk = c; pc.group = ngroups;
        pc.ring_off = o * out;
        pc.src_off = src0 + (g0 + o) * rec;
        pc.items = b;
        pc.last_of_group = o + b == gi;
        pc.last_of_chunk = pc.last_of_group && g0 + gi == items;
        pc.group_dst_off = g0 * out;
        pc.group_bytes = gi * out;
        // (what the ring and the HBM buffers rely on, checked where it is decided: a piece ends inside its group's ring slot,
        // a group inside its chunk's buffer)
        if (pc.ring_off + b * out > F.kSlotBytes || pc.group_bytes > F.kSlotBytes || pc.group_dst_off + pc.group_bytes > items * out)
          return fail("internal: feed plan outside the ring slot / chunk buffer");
        pieces.push_back(pc);
        o += b;
      }
      g0 += gi;
      ngroups++;
    }
  }
  F.begin(pieces, mem, fd, packed, rec, skip);
  struct End {
    Feeder &f;
    ~End() { f.end(); }
  } end_guard{F};
  size_t issued = 0, released = 0;  // in groups
  auto release_done = [&]() {  // DMAs that have finished: their ring slots may be refilled
    while (released < issued && hipEventQuery(F.sent[released % Feeder::kSlots]) == hipSuccess) released++;
    F.released.store(released, std::memory_order_release);
  };
  bool chunk_open = false;  // a group of the current chunk has been sent already
  for (size_t p = 0; p < pieces.size(); p++) {
    const Feeder::Piece &pc = pieces[p];
    const int c = pc.chunk, slot = c % nslots;
    uint8_t st;
    while ((st = F.filled[p].load(std::memory_order_acquire)) == 0) {
      release_done();
      std::this_thread::yield();
    }
    if (st != 1) {
      F.abort = true;
      return fail("input file: read error");
    }
    if (!pc.last_of_group) continue;
    const int base = plan[c], m = plan[c + 1] - plan[c];
    uint8_t *chunk_dst = r.d_images[slot];
    // the chunk that had this HBM buffer before: its stages are done (both DMA queues write the buffer)
    if (!chunk_open && c >= nslots) {
      HIP_OK(hipStreamWaitEvent(r.copy_stream, r.consumed[slot], 0));
      if (F.aux) HIP_OK(hipStreamWaitEvent(F.aux, r.consumed[slot], 0));
    }
    chunk_open = !pc.last_of_chunk;
    hipStream_t ds = (F.aux && (pc.group & 1)) ? F.aux : r.copy_stream;
    HIP_OK(hipMemcpyAsync(chunk_dst + pc.group_dst_off, F.ring + (size_t)(pc.group % Feeder::kSlots) * F.kSlotBytes, pc.group_bytes, hipMemcpyHostToDevice, ds));
    HIP_OK(hipEventRecord(F.sent[pc.group % Feeder::kSlots], ds));
    issued = (size_t)pc.group + 1;
    release_done();
    if (!pc.last_of_chunk) continue;
    if (F.aux) {  // the chunk is complete when both queues have delivered their groups
      HIP_OK(hipEventRecord(F.aux_done, F.aux));
      HIP_OK(hipStreamWaitEvent(r.copy_stream, F.aux_done, 0));
    }
    HIP_OK(hipEventRecord(r.copied[slot], r.copy_stream));
    HIP_OK(hipStreamWaitEvent(lane_stream(c, lanes), r.copied[slot], 0));
    if (consume(c, base, m, slot)) return -1;
    // (only where a later chunk will reuse this buffer: a marker packet on the lane's stream is not free, BNN_MI355X_TRACE)
    if (c + nslots < nchunks) HIP_OK(hipEventRecord(r.consumed[slot], lane_stream(c, lanes)));
  }
  return 0;
}

// First use of a process: the first launch of a kernel pays for loading its code object and for the
// allocation of workspace and events, and all of that would land in the `usecPerImage` of the caller's first
// inference() (measured: 2.4 ms instead of ~10 us for one lfcW1A1 image; the reference's FPGA reports 7-8 us
// from the first call on).  So the load pays it: one image through the small-batch kernels and a few
// thousand through the throughput forms, zeros in, results dropped.  Once per process.
int warm_up() {
  Runtime &r = rt();
  if (r.warmed || std::getenv("BNN_MI355X_NO_WARMUP")) return 0;
  const int big = 8192;
  const size_t isz = (size_t)r.spec.image_bytes();
  if (reserve(big) || reserve_host(big, (size_t)big)) return -1;
  // (the pinned ring and the reader threads of the file path are NOT created here: 48 MB of pinned memory and six threads
  // per loaded network would be a poor default for users who never classify a large file; the first such call pays ~10 ms)
  HIP_OK(hipMemsetAsync(r.d_images[0], 0, (size_t)big * isz, r.stream));
  for (int n : {1, 2, 300, 600, 1100, 2500, 5000, big})  // one batch size inside every band of the dispatch policy
    if (enqueue(r.d_images[0], n, 10, r.d_classes, r.spec.is_cnv ? r.d_scores : nullptr, r.d_words, r.stream)) return -1;
  if (r.spec.is_cnv) {  // the file path's label-stripping kernel lives in another code object
    const hipError_t e = launch_strip_records(r.d_images[0], 3073, 1, r.d_images[1], 2, r.stream);
    if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
  } else {  // the forms that start from host-binarised words (the zeros read as 13-word images just as well)
    for (int n : {1, 300, 600, 1100, 2500, big})
      if (enqueue(r.d_images[0], n, 10, r.d_classes, nullptr, r.d_words, r.stream, nullptr, nullptr, 0, false, true)) return -1;
  }
  // the pinned I/O block of the direct calls, and one image through it
  if (ensure_io()) return -1;
  {
    const ResultSlots m = mapped_results(1, r.spec.is_cnv, true);
    if (m.d_classes && enqueue(r.spec.is_cnv ? r.d_io + 16 : r.d_io, 1, 10, m.d_classes, m.d_scores, m.d_words, r.stream, r.io_t0, r.io_t1, 0, true, !r.spec.is_cnv))
      return -1;
  }
  while (r.time_events.size() < 2) {
    hipEvent_t e;
    HIP_OK(hipEventCreateWithFlags(&e, kTimeEventFlags));
    r.time_events.push_back(e);
  }
  HIP_OK(hipEventRecord(r.time_events[0], r.stream));
  HIP_OK(hipEventRecord(r.time_events[1], r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  r.warmed = true;
  return 0;
}

// ---- input files, streamed ---------------------------------------------------
// CIFAR-10 binary: records of [label u8][R 1024][G 1024][B 1024] (tiny-cnn parse_cifar10, call site
// main_python.cpp:129,152); bodies go to the GPU as they are, planar CHW uint8.  MNIST idx3: 16-byte
// big-endian header (magic 0x803, count, rows, cols), then count x 784 uint8 (tiny-cnn
// parse_mnist_images, lfcW1A1/sw/main_python.cpp:122,144).
// The entry points do not parse the file on the host: the records go to HBM as they lie on
// disk (reader threads pread() chunk c+1 while chunk c is copied and classified) and the label
// bytes are dropped by a kernel (k_strip_records).  An MNIST body needs no kernel at all.
struct ImageFile {
  int fd = -1;
  size_t n = 0;            // images
  size_t rec = 0, skip = 0;  // bytes per record on disk, bytes to drop at the start of each
  size_t first = 0;        // file offset of record 0
  ~ImageFile() { if (fd >= 0) ::close(fd); }
};

int open_image_file(const char *path, ImageFile &f) {
  Runtime &r = rt();
  f.fd = ::open(path ? path : "", O_RDONLY);
  struct stat st;
  if (f.fd < 0 || ::fstat(f.fd, &st) != 0) return fail(std::string("Could not open file ") + (path ? path : ""));
  const size_t size = (size_t)st.st_size;
  if (r.spec.is_cnv) {  // whole records only, a trailing partial record is ignored (the reference reads record by record)
    f.rec = 3073; f.skip = 1; f.first = 0;
    f.n = size / 3073;
  } else {
    unsigned char h[16];
    if (::pread(f.fd, h, 16, 0) != 16) return fail("MNIST image file: short header");
    auto be = [&](int o) { return ((uint32_t)h[o] << 24) | ((uint32_t)h[o + 1] << 16) | ((uint32_t)h[o + 2] << 8) | h[o + 3]; };
    if (be(0) != 0x803u || be(8) != 28 || be(12) != 28) return fail("MNIST image file: bad header");
    f.rec = 784; f.skip = 0; f.first = 16;
    f.n = be(4);
    if (size < 16 + f.n * 784) return fail("MNIST image file: truncated");
  }
  if (f.n > 0x7FFFFFFFu) return fail("input file: too many images for the int-sized ABI");
  return 0;
}

// pread() [offset, offset + bytes) into dst on up to 8 threads (a single thread moves page-cache
// data at a fraction of what the PCIe link takes)
struct ChunkReader {
  std::vector<std::thread> threads;
  std::atomic<bool> ok{true};
  void start(int fd, size_t offset, size_t bytes, uint8_t *dst) {
    ok = true;
    const size_t hw = std::thread::hardware_concurrency();
    size_t nt = bytes / (4u << 20) + 1;
    if (nt > 8) nt = 8;
    if (hw && nt > hw) nt = hw;
    if (nt == 1) {  // small read: not worth a thread
      size_t done = 0;
      while (done < bytes) {
        const ssize_t got = ::pread(fd, dst + done, bytes - done, (off_t)(offset + done));
        if (got <= 0) { ok = false; return; }
        done += (size_t)got;
      }
      return;
    }
    const size_t part = ((bytes + nt - 1) / nt + 4095) & ~(size_t)4095;
    for (size_t t = 0; t < nt; t++) {
      const size_t lo = t * part, hi = (lo + part < bytes) ? lo + part : bytes;
      if (lo >= hi) break;
      threads.emplace_back([this, fd, offset, dst, lo, hi] {
        size_t done = lo;
        while (done < hi) {
          const ssize_t got = ::pread(fd, dst + done, hi - done, (off_t)(offset + done));
          if (got <= 0) { ok = false; return; }
          done += (size_t)got;
        }
      });
    }
  }
  bool wait() {
    for (auto &t : threads) t.join();
    threads.clear();
    return ok;
  }
  ~ChunkReader() { (void)wait(); }
};

// Streams images [0, n) of an open file into HBM, chunk by chunk (plan_chunks; reader
// threads one chunk ahead of the copy).  Chunk c lands packed (labels stripped) at dst(base, slot) and
// `consume(c, base, m, slot)` is called once its copy and strip are enqueued on copy_stream and
// the chunk's lane (lane_stream(c, lanes)) has been made to wait for them.  reuse_slots: the destinations alternate between two
// buffers, so a chunk's copy must wait until the stages of the chunk two before have consumed it.
template <typename Dst, typename Consume>
int stream_file(const ImageFile &f, int n, bool reuse_slots, int lanes, Dst dst, Consume consume) {
  Runtime &r = rt();
  const std::vector<int> plan = plan_chunks(n, false, true);
  const int chunk = largest_chunk(plan);
  const int nchunks = (int)plan.size() - 1;
  const size_t chunk_bytes = (size_t)chunk * f.rec;
  if (chunk_bytes > r.file_cap) {
    HIP_OK(hipDeviceSynchronize());
    for (int i = 0; i < 2; i++) {
      (void)hipFree(r.d_file[i]);
      r.d_file[i] = nullptr;
      r.h_file[i].reset();
    }
    r.file_cap = 0;
    for (int i = 0; i < 2; i++) {
      r.h_file[i].reset(new (std::nothrow) uint8_t[chunk_bytes + 8]);
      if (!r.h_file[i]) return fail("out of memory");
      if (f.skip) HIP_OK(hipMalloc(reinterpret_cast<void **>(&r.d_file[i]), chunk_bytes + 256));
      if (!r.file_sent[i]) HIP_OK(hipEventCreateWithFlags(&r.file_sent[i], hipEventDisableTiming));
    }
    r.file_cap = chunk_bytes;
  }
  ChunkReader reader;
  auto span = [&](int c, size_t *off, int *m) {
    *m = plan[c + 1] - plan[c];
    *off = f.first + (size_t)plan[c] * f.rec;
  };
  size_t off;
  int m;
  span(0, &off, &m);
  reader.start(f.fd, off, (size_t)m * f.rec, r.h_file[0].get());
  for (int c = 0; c < nchunks; c++) {
    const int base = plan[c], slot = c & 1;
    span(c, &off, &m);
    if (!reader.wait()) return fail("input file: read error");
    if (c + 1 < nchunks) {  // the other host chunk is free once its copy (chunk c-1) has left it
      if (c >= 1) HIP_OK(hipEventSynchronize(r.file_sent[slot ^ 1]));
      size_t off2;
      int m2;
      span(c + 1, &off2, &m2);
      reader.start(f.fd, off2, (size_t)m2 * f.rec, r.h_file[slot ^ 1].get());
    }
    // one chunk: nothing to overlap, stay on the compute stream (fewer driver round trips for small calls)
    hipStream_t cs = (nchunks == 1 && reuse_slots) ? r.stream : r.copy_stream;
    if (c >= 2) HIP_OK(hipStreamWaitEvent(cs, r.consumed[slot], 0));  // d_file[slot] / dst free again
    uint8_t *packed = dst(base, slot);
    uint8_t *to = f.skip ? r.d_file[slot] : packed;
    HIP_OK(hipMemcpyAsync(to, r.h_file[slot].get(), (size_t)m * f.rec, hipMemcpyHostToDevice, cs));
    if (nchunks > 1) HIP_OK(hipEventRecord(r.file_sent[slot], cs));
    if (f.skip) {
      const hipError_t e = launch_strip_records(r.d_file[slot], (int)f.rec, (int)f.skip, packed, m, cs);
      if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
    }
    if (cs != r.stream) {
      HIP_OK(hipEventRecord(r.copied[slot], cs));
      HIP_OK(hipStreamWaitEvent(lane_stream(c, lanes), r.copied[slot], 0));
    }
    if (consume(c, base, m, slot)) return -1;
    // (with reuse_slots the consumer's stages read `packed`; without, only the strip kernel reads d_file[slot])
    if (c + 2 < nchunks) HIP_OK(hipEventRecord(r.consumed[slot], reuse_slots ? lane_stream(c, lanes) : r.copy_stream));
  }
  return 0;
}

// ---- host buffers: the copies on a thread of their own -------------------------------------------------------
// hipMemcpyAsync from PAGEABLE memory returns when the bytes have left (the runtime pins or stages the pages and waits for
// its DMA): with copies and launches on one thread the link idles while the nine launches of every chunk are enqueued --
// 20-45 us a chunk, 150-250 us of a 1.2 ms call of 10 000 CIFAR images (BNN_MI355X_TRACE: the copies alone ran at
// 28-52 GB/s, the call's bytes arrived at 37).  So the copies of chunks 1.. are issued by a helper thread, back to back
// on the copy stream, while the calling thread enqueues stages; chunk 0's copy stays with the caller (the helper needs
// 30-60 us to wake up).  Two counters tie them together: `copied` (helper -> caller: chunks whose `copied` event is
// recorded -- a stream may only be made to wait for an event that has been recorded) and `consumed` (caller -> helper:
// chunks whose stages are enqueued and whose `consumed` event is recorded -- their HBM slot may be overwritten).
// One per process, never destroyed (like the feeder's threads).
struct Copier {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv, cv_idle;
  bool started = false, busy = false;
  uint64_t job_id = 0;
  // the job
  const uint8_t *src = nullptr;
  const std::vector<int> *plan = nullptr;
  size_t isz = 0;
  int nslots = 2, device = 0;
  std::atomic<int> copied{0}, consumed{0};
  std::atomic<bool> abort{false}, failed{false};
  std::string err;

  void run() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return job_id != seen; });
        seen = job_id;
      }
      Runtime &r = rt();
      const int nchunks = (int)plan->size() - 1;
      hipError_t e = hipSetDevice(device);
      for (int c = 1; c < nchunks && e == hipSuccess; c++) {
        const int slot = c % nslots, base = (*plan)[c], m = (*plan)[c + 1] - base;
        // chunk c-1's copy is in the stream (the caller's for c = 1), and the chunk that had this slot is consumed
        while (!abort.load(std::memory_order_relaxed) &&
               (copied.load(std::memory_order_acquire) < c || (c >= nslots && consumed.load(std::memory_order_acquire) < c - nslots + 1)))
          std::this_thread::yield();
        if (abort.load(std::memory_order_relaxed)) break;
        if (c >= nslots) e = hipStreamWaitEvent(r.copy_stream, r.consumed[slot], 0);
        if (e == hipSuccess) e = hipMemcpyAsync(r.d_images[slot], src + (size_t)base * isz, (size_t)m * isz, hipMemcpyHostToDevice, r.copy_stream);
        if (e == hipSuccess) e = hipEventRecord(r.copied[slot], r.copy_stream);
        if (e == hipSuccess) copied.store(c + 1, std::memory_order_release);
      }
      if (e != hipSuccess) {
        err = std::string("host buffer copy: ") + hipGetErrorString(e);
        failed.store(true, std::memory_order_release);
      }
      std::lock_guard<std::mutex> lk(mu);
      busy = false;
      cv_idle.notify_all();
    }
  }
  void begin(const uint8_t *s, const std::vector<int> &p, size_t image_bytes, int slots, int dev) {
    std::lock_guard<std::mutex> lk(mu);
    if (!started) {
      th = std::thread([this] { run(); });
      th.detach();
      started = true;
    }
    src = s; plan = &p; isz = image_bytes; nslots = slots; device = dev;
    copied = 0; consumed = 0; abort = false; failed = false;
    busy = true;
    job_id++;
    cv.notify_one();
  }
  // the helper has left the job: its description may go out of scope
  void end() {
    abort = true;  // (a no-op after a complete run)
    std::unique_lock<std::mutex> lk(mu);
    cv_idle.wait(lk, [&] { return !busy; });
  }
};
Copier &copier() {
  static Copier *c = new Copier;
  return *c;
}

// ---- the entry points that take HOST data --------------------------------------------------------------------
// n images from host memory (mem) or from an open input file -> any of classes / scores / words (host arrays).
// usec: device time of the compute stages only, per image (the reference times the accelerator call alone,
// foldedmv-offload.h:389-392, and excludes the transfers: TRANSFER_EXCL, foldedmv-offload.cpp:53-61).
struct Source {
  const uint8_t *mem = nullptr;     // n x image_bytes, as in the bodies of the file formats, or
  const ImageFile *file = nullptr;  // an open CIFAR-10 binary / MNIST idx3 file
};

// Small calls -- one CIFAR image (classify_image and the webcam loops call inference(path) per frame,
// bnn/bnn.py:131-137, main_python.cpp:120-139), up to kDirectMaxLfc MNIST images -- with no transfer at all: the image
// (LFC: binarised here, 13 words each, like the reference's host does) is placed in pinned memory the GPU addresses,
// the one-launch kernels read it over the link and write their results into pinned memory: launch, one wait.
// words_view (optional, LFC): receives a pointer to the raw output words where the call left them in pinned memory,
// valid until the next call into the library -- the batched decode reads them there instead of from a copy
int infer_direct(const Source &src, int n, int ncls, int32_t *classes, int16_t *scores, uint64_t *words, float *usec, const uint64_t **words_view) {
  Runtime &r = rt();
  if (ensure_io() || reserve(n)) return -1;
  trace().mark("reserved");
  const uint8_t *d_in = r.d_io;
  if (r.spec.is_cnv) {
    // the kernels read an image with 128-bit loads: the body (3072 bytes behind the label byte) starts at +16
    if (src.file) {  // (n == 1: the records of a file are a label byte apart)
      if (::pread(src.file->fd, r.h_io + 15, 3073, (off_t)src.file->first) != 3073) return fail("input file: read error");
    } else {
      std::memcpy(r.h_io + 16, src.mem, (size_t)n * 3072);
    }
    d_in = r.d_io + 16;
  } else if (src.file) {
    const size_t bytes = (size_t)n * kLfcPixels;
    if (r.h_scratch.size() < bytes) r.h_scratch.resize(bytes);
    size_t done = 0;
    while (done < bytes) {
      const ssize_t got = ::pread(src.file->fd, r.h_scratch.data() + done, bytes - done, (off_t)(src.file->first + done));
      if (got <= 0) return fail("input file: read error");
      done += (size_t)got;
    }
    binarize_pack(r.h_scratch.data(), (size_t)n, reinterpret_cast<uint64_t *>(r.h_io));
  } else {
    binarize_pack(src.mem, (size_t)n, reinterpret_cast<uint64_t *>(r.h_io));
  }
  const bool want_scores = scores && r.spec.is_cnv;
  const ResultSlots m = mapped_results(n, want_scores, true);
  if (!m.d_classes) return fail("pinned I/O block unavailable");
  DrainOnFailure drain;
  trace().mark("input_placed");
  // BNN_MI355X_DIRECT_TIMING=host (opt-in, one image): the call is timed and waited for WITHOUT the runtime -- no event
  // packets around the launch, the last kernel stores a completion word into the pinned block behind its results, the host
  // spins on that word, and usecPerImage is the host's clock from the launch to the word, i.e. the reference's own
  // definition (wall clock around the accelerator call, foldedmv-offload.cpp:138-140, foldedmv-offload.h:342-345) instead of this runtime's (device
  // time by events).  tools/launch_latency_probe.hip, profiles/r04_launch_latency_probe.txt: the two timing events cost
  // 4.3 us in the launch call and ~2 us in a later kernel start, the event's readiness is seen ~2 us after the word:
  // 21.5 -> 13.9 us around an 8 us kernel.  The default keeps the events: usecPerImage keeps its meaning.
  static const bool host_timing = [] { const char *e = std::getenv("BNN_MI355X_DIRECT_TIMING"); return e && std::strcmp(e, "host") == 0; }();
  if (host_timing && n == 1) {
    volatile unsigned *done = reinterpret_cast<volatile unsigned *>(r.h_io + kIoDoneOff);
    const unsigned seq = ++r.io_seq;
    const auto t_launch = std::chrono::steady_clock::now();
    if (enqueue(d_in, n, ncls, classes ? m.d_classes : nullptr, want_scores ? m.d_scores : nullptr, m.d_words, r.stream, nullptr, nullptr, 0, false,
                !r.spec.is_cnv, reinterpret_cast<unsigned *>(r.d_io + kIoDoneOff), seq))
      return -1;
    trace().mark("launched");
    const auto until = t_launch + std::chrono::microseconds(500);
    while (*done != seq && std::chrono::steady_clock::now() < until) {}
    auto t_done = std::chrono::steady_clock::now();
    if (*done != seq) {
      // not within 500 us: something else holds the GPU -- or this pass has no one-block last kernel to set the mark (a
      // cnvW2A2 under fault injection runs its -2-aware staged layers): the blocking wait, the results are there after it
      HIP_OK(hipStreamSynchronize(r.stream));
      t_done = std::chrono::steady_clock::now();
    }
    trace().mark("synced");
    if (classes) std::memcpy(classes, m.h_classes, (size_t)n * 4);
    if (want_scores) std::memcpy(scores, m.h_scores, (size_t)n * 128);
    if (words && !r.spec.is_cnv) std::memcpy(words, m.h_words, (size_t)n * 8);
    if (words_view) *words_view = m.h_words;
    if (usec) *usec = std::chrono::duration<float, std::micro>(t_done - t_launch).count();
    drain.ok();
    trace().mark("done");
    trace().dump("direct, host-timed");
    return 0;
  }
  if (enqueue(d_in, n, ncls, classes ? m.d_classes : nullptr, want_scores ? m.d_scores : nullptr, m.d_words, r.stream, r.io_t0, r.io_t1, 0, true,
              !r.spec.is_cnv))
    return -1;
  trace().mark("launched");
  // The wait: a blocking wait sleeps until the completion interrupt has made its way to this thread -- 15-25 us behind a
  // 9 us kernel (BNN_MI355X_TRACE).  For calls this small the thread polls the stop event instead, for at most 300 us;
  // whatever is not done by then gets the blocking wait.
  {
    const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(300);
    hipError_t q;
    while ((q = hipEventQuery(r.io_t1)) == hipErrorNotReady && std::chrono::steady_clock::now() < until) {}
    if (q != hipSuccess) HIP_OK(hipStreamSynchronize(r.stream));
  }
  trace().mark("synced");
  if (classes) std::memcpy(classes, m.h_classes, (size_t)n * 4);
  if (want_scores) std::memcpy(scores, m.h_scores, (size_t)n * 128);
  if (words && !r.spec.is_cnv) std::memcpy(words, m.h_words, (size_t)n * 8);
  if (words_view) *words_view = m.h_words;
  float ms = 0.f;
  HIP_OK(hipEventElapsedTime(&ms, r.io_t0, r.io_t1));
  if (usec) *usec = ms * 1000.f / (float)n;
  drain.ok();
  trace().mark("done");
  trace().dump("direct");
  return 0;
}

int infer_any(const Source &src, int n, int ncls, int32_t *classes, int16_t *scores, uint64_t *words, float *usec, const uint64_t **words_view = nullptr) {
  Runtime &r = rt();
  if (!ready()) return -1;
  if (bad_number_class(ncls)) return -1;
  if (usec) *usec = 0.f;
  if (n <= 0) return 0;
  if (!src.file) trace().start();  // (a file call started the clock before it opened the file)
  const bool from_file = src.file != nullptr;
  const bool hook = r.debug_last_stage >= 0;  // (the stage-output test hook reads the workspace after the call: all images in it, one chunk, device binarisation)
  const bool want_scores = scores && r.spec.is_cnv;
  static const bool no_direct = std::getenv("BNN_MI355X_NO_DIRECT") != nullptr;  // A/B
  if (!hook && !r.profiling && !no_direct && n <= (r.spec.is_cnv ? (from_file ? 1 : kDirectMaxCnv) : kDirectMaxLfc) && (!want_scores || n <= kMappedScoresMax))
    return infer_direct(src, n, ncls, classes, scores, words, usec, words_view);
  const size_t isz = (size_t)r.spec.image_bytes();
  const size_t rec = from_file ? src.file->rec : isz, skip = from_file ? src.file->skip : 0, first = from_file ? src.file->first : 0;
  const std::vector<int> plan = plan_chunks(n, hook, from_file);
  const int chunk = largest_chunk(plan);
  const int nchunks = (int)plan.size() - 1;
  // LFC: binarizeAndPack on the host side of the copy, as the reference does (foldedmv-offload.cpp:82-98,186-194): worker
  // threads turn 784 pixels into 13 words straight into pinned memory and 104 bytes per image cross the link (the raw pixels
  // made every host-path call of the LFC nets PCIe-bound at 34-37 GB/s = 43 M images/s, against 230 M/s of stages).
  static const bool no_pack = std::getenv("BNN_MI355X_NO_HOST_PACK") != nullptr;  // A/B: raw pixels to HBM, binarised there
  const bool packed = !r.spec.is_cnv && !hook && !no_pack && feeder().init() == 0 && (size_t)chunk * kLfcWords * 8 <= feeder().kSlotBytes;
  // The pinned ring is for FILES (and for the LFC nets' binarised words).  A CIFAR buffer in host memory goes faster without
  // it: the runtime's own pageable path moves a 100 MB chunk at 54 GB/s (profiles/r03_h2d_probe.txt), the ring's 4-8 MB
  // pieces reach 49-52 and add a copy (measured, same box: 13.8 ms through the ring, 12.7 ms without, 131 072 CIFAR
  // images).  BNN_MI355X_FEED_HOST=1 forces it.
  static const bool feed_host = std::getenv("BNN_MI355X_FEED_HOST") != nullptr;
  // large file: worker threads pread() it into the pinned ring piece by piece (feed_chunks); small: one or a few chunks
  // through a pageable host chunk (stream_file) -- also where the ring cannot be had (no pinned memory to spare): slower, same result
  const bool ring = packed || ((from_file || feed_host) && nchunks > 1 && use_feeder((size_t)n * rec) && feeder().init() == 0);
  const int lanes = lanes_for(nchunks);
  const int nslots = slots_for(lanes);
  if (reserve(chunk) || (lanes == 2 && reserve2(chunk)) || reserve_host(chunk, (size_t)n, nslots)) return -1;
  while ((int)r.time_events.size() < 2 * nchunks) {
    hipEvent_t e;
    HIP_OK(hipEventCreateWithFlags(&e, kTimeEventFlags));
    r.time_events.push_back(e);
  }
  // results: small calls have the last stage write them into pinned memory (no copy back); larger ones keep them in HBM
  // and fetch them with ONE transfer at the end (a D2H into pageable memory per chunk would make the host wait for each
  // chunk's kernels before it can queue the next copy)
  const ResultSlots m = hook ? ResultSlots{} : mapped_results(n, want_scores);
  int32_t *const dc = m.d_classes ? m.d_classes : r.d_classes;
  uint64_t *const dw = m.d_words ? m.d_words : r.d_words;
  int16_t *const ds = m.d_scores ? m.d_scores : r.d_scores;
  const bool want_words = (words || words_view) && !r.spec.is_cnv;
  if (classes && !m.d_classes && grow_pinned(r.h_classes, r.h_classes_cap, (size_t)n)) return -1;
  if (want_words && !m.d_words && grow_pinned(r.h_words, r.h_words_cap, (size_t)n)) return -1;
  DrainOnFailure drain;
  trace().mark("reserved");
  // (experiment switch, read per call so that tools/plan_ab.py can interleave it: no timing events around the chunks,
  // usecPerImage reported as 0 -- what the two marker packets per chunk cost a device-bound call)
  const bool timed = std::getenv("BNN_MI355X_NO_CHUNK_TIMING") == nullptr;
  auto stages = [&](int c, int base, int mm, int slot) {
    trace().mark("chunk_in", c);
    const int rc = enqueue(r.d_images[slot], mm, ncls, classes ? dc + base : nullptr, want_scores ? ds + (size_t)base * 64 : nullptr, dw + base,
                           lane_stream(c, lanes), timed ? r.time_events[2 * c] : nullptr, timed ? r.time_events[2 * c + 1] : nullptr,
                           lanes == 2 ? (c & 1) : 0, nchunks == 1, packed);
    trace().mark("queued", c);
    return rc;
  };
  if (ring) {
    if (feed_chunks(src.mem, from_file ? src.file->fd : -1, first, rec, skip, plan, lanes, packed, stages)) return -1;
  } else if (from_file) {
    if (stream_file(*src.file, n, true, lanes, [&](int, int slot) { return r.d_images[slot]; }, stages)) return -1;
  } else if (nchunks == 1) {  // nothing to overlap: stay on one stream (fewer driver round trips for small calls)
    HIP_OK(hipMemcpyAsync(r.d_images[0], src.mem, (size_t)n * isz, hipMemcpyHostToDevice, r.stream));
    if (stages(0, 0, n, 0)) return -1;
  } else {
    static const bool one_thread = std::getenv("BNN_MI355X_NO_COPIER") != nullptr;  // A/B: copies and launches on the calling thread
    Copier &K = copier();
    struct End {
      Copier *k;
      ~End() { if (k) k->end(); }
    } end_guard{one_thread ? nullptr : &K};
    if (!one_thread) K.begin(src.mem, plan, isz, nslots, r.device);  // (copies of chunks 1..: "the copies on a thread of their own" above)
    for (int c = 0; c < nchunks; c++) {
      const int base = plan[c], mm = plan[c + 1] - plan[c], slot = c % nslots;
      if (one_thread || c == 0) {
        if (c >= nslots) HIP_OK(hipStreamWaitEvent(r.copy_stream, r.consumed[slot], 0));
        HIP_OK(hipMemcpyAsync(r.d_images[slot], src.mem + (size_t)base * isz, (size_t)mm * isz, hipMemcpyHostToDevice, r.copy_stream));
        HIP_OK(hipEventRecord(r.copied[slot], r.copy_stream));
        if (!one_thread) K.copied.store(1, std::memory_order_release);
      } else {
        while (K.copied.load(std::memory_order_acquire) <= c) {
          if (K.failed.load(std::memory_order_acquire)) return fail(K.err);
          std::this_thread::yield();
        }
      }
      HIP_OK(hipStreamWaitEvent(lane_stream(c, lanes), r.copied[slot], 0));
      if (stages(c, base, mm, slot)) return -1;
      if (c + nslots < nchunks) HIP_OK(hipEventRecord(r.consumed[slot], lane_stream(c, lanes)));  // (a later chunk reuses the slot)
      if (!one_thread) K.consumed.store(c + 1, std::memory_order_release);
    }
  }
  if (join_lanes(lanes)) return -1;
  trace().mark("all_queued");
  if (classes && !m.d_classes) HIP_OK(hipMemcpyAsync(r.h_classes, r.d_classes, (size_t)n * 4, hipMemcpyDeviceToHost, r.stream));
  if (want_scores && !m.d_scores) HIP_OK(hipMemcpyAsync(scores, r.d_scores, (size_t)n * 128, hipMemcpyDeviceToHost, r.stream));
  if (want_words && !m.d_words) HIP_OK(hipMemcpyAsync(r.h_words, r.d_words, (size_t)n * 8, hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  if (from_file) HIP_OK(hipStreamSynchronize(r.copy_stream));
  trace().mark("synced");
  if (classes) std::memcpy(classes, m.d_classes ? m.h_classes : r.h_classes, (size_t)n * 4);
  if (want_scores && m.d_scores) std::memcpy(scores, m.h_scores, (size_t)n * 128);
  if (words && !r.spec.is_cnv) std::memcpy(words, m.d_words ? m.h_words : r.h_words, (size_t)n * 8);
  if (words_view) *words_view = m.d_words ? m.h_words : r.h_words;
  double total_ms = 0.0;
  if (timed && chunks_device_ms(nchunks, &total_ms)) return -1;
  if (usec) *usec = (float)(total_ms * 1000.0 / n);
  drain.ok();
  trace().mark("done");
  trace().dump(ring ? (packed ? "ring, host-binarised" : "ring") : (from_file ? "pageable file chunks" : "pageable buffer"));
  return 0;
}
int infer_host(const uint8_t *imgs, int n, int ncls, int32_t *classes, int16_t *scores, uint64_t *words, float *usec, const uint64_t **words_view = nullptr) {
  Source s;
  s.mem = imgs;
  return infer_any(s, n, ncls, classes, scores, words, usec, words_view);
}
int infer_file(const ImageFile &f, int n, int ncls, int32_t *classes, int16_t *scores, uint64_t *words, float *usec, const uint64_t **words_view = nullptr) {
  Source s;
  s.file = &f;
  return infer_any(s, n, ncls, classes, scores, words, usec, words_view);
}

// all images of a file, packed, resident in HBM at r.d_all (fault campaigns classify them in runs)
int load_file_resident(const ImageFile &f, int n) {
  Runtime &r = rt();
  const size_t isz = (size_t)r.spec.image_bytes();
  if (bind_device() || r.d_all.grow((size_t)n * isz + 256)) return -1;
  DrainOnFailure drain;
  if (stream_file(
          f, n, false, 1, [&](int base, int) { return r.d_all + (size_t)base * isz; }, [&](int, int, int, int) { return 0; }))
    return -1;
  HIP_OK(hipStreamSynchronize(r.copy_stream));
  drain.ok();
  return 0;
}

// ---- LFC host decode (libm, like the reference) -------------------------------
uint64_t label_mask(int ncls) { return 0xFFFFFFFFFFFFFFFFull >> (64 - ncls); }
// batched: (unsigned) log2((double) word), 0 when no bit is set (foldedmv-offload.cpp:213-220)
int lfc_class_batched(uint64_t w, int ncls) {
  w &= label_mask(ncls);
  // below 2^47 the double-precision log2 cannot round up to the next integer (2^k - 1 lies 1.44 * 2^-k below k, an ulp
  // of k is 2^-47 for k >= 32): its truncation IS the index of the highest set bit -- without 131 072 calls into libm
  // per LFC batch (0.8 ms of a 1.9 ms call, BNN_MI355X_TRACE).  Wider words go through libm like the reference's.
  if ((w >> 47) == 0) return w ? 63 - __builtin_clzll(w) : 0;
  return (int)(unsigned int)std::log2((double)w);
}
// single: index of the one-hot entry = round(log2(word)) (foldedmv-offload.cpp:152-165)
int lfc_hot_single(uint64_t w, int ncls) {
  w &= label_mask(ncls);
  return w ? (int)(unsigned int)std::round(std::log2((double)w)) : 0;
}

// the result array of inference_multiple: class indices, or (CNV, enable_detail) number_class scores
// per image.  `infer(classes, scores, words)` runs the batch from wherever the images are.
template <typename Infer>
int *classify_with(Infer infer, int n, int ncls, int enable_detail) {
  Runtime &r = rt();
  int *result = nullptr;
  if (r.spec.is_cnv && enable_detail) {
    std::vector<int16_t> s((size_t)n * 64);
    if (infer(nullptr, s.data(), nullptr, nullptr)) return nullptr;
    result = new (std::nothrow) int[(size_t)(n > 0 ? n : 1) * ncls];
    if (!result) { fail("out of memory"); return nullptr; }
    for (int i = 0; i < n; i++)
      for (int j = 0; j < ncls; j++) result[(size_t)i * ncls + j] = s[(size_t)i * 64 + j];
  } else if (r.spec.is_cnv) {
    result = new (std::nothrow) int[(size_t)(n > 0 ? n : 1)];
    if (!result) { fail("out of memory"); return nullptr; }
    if (infer(result, nullptr, nullptr, nullptr)) { delete[] result; return nullptr; }
  } else if (ncls <= 47) {
    // the LFC libraries ignore enable_detail (lfcW1A1/sw/main_python.cpp:135-156).  Up to 47 classes the reference's
    // (unsigned) log2((double) word) IS the index of the highest set bit (lfc_class_batched above), which the last stage
    // computes on the device: the classes come back as they are, no pass over 131 072 words on the host after the wait
    result = new (std::nothrow) int[(size_t)(n > 0 ? n : 1)];
    if (!result) { fail("out of memory"); return nullptr; }
    if (infer(result, nullptr, nullptr, nullptr)) { delete[] result; return nullptr; }
  } else {
    const uint64_t *w = nullptr;  // the raw output words, where the call left them (pinned memory)
    if (infer(nullptr, nullptr, nullptr, &w)) return nullptr;
    result = new (std::nothrow) int[(size_t)(n > 0 ? n : 1)];
    if (!result) { fail("out of memory"); return nullptr; }
    for (int i = 0; i < n; i++) result[i] = lfc_class_batched(w[i], ncls);
  }
  return result;
}

int *classify_host(const uint8_t *imgs, int n, int ncls, float *usec, int enable_detail) {
  return classify_with([&](int32_t *c, int16_t *s, uint64_t *w, const uint64_t **v) { return infer_host(imgs, n, ncls, c, s, w, usec, v); }, n, ncls,
                       enable_detail);
}

// a bnn_mi355x_last_* getter: the first `cap` values into the caller's array (which may be null); returns how many there are
template <class T>
int copy_out(const std::vector<T> &v, T *out, int cap) {
  for (int i = 0; out && i < cap && i < (int)v.size(); i++) out[i] = v[(size_t)i];
  return (int)v.size();
}

// ---- what the picture entry points share ----------------------------------------------------------------------------

// Enqueues on r.stream the upload of `height` rows of row_bytes to packed rows at dst: one flat copy when the source is
// packed (row_stride 0 or row_bytes), else a 2-D one
int upload_rows(uint8_t *dst, const uint8_t *pixels, size_t row_bytes, long row_stride, int height) {
  Runtime &r = rt();
  if (row_stride == 0 || (size_t)row_stride == row_bytes)
    HIP_OK(hipMemcpyAsync(dst, pixels, row_bytes * height, hipMemcpyHostToDevice, r.stream));
  else
    HIP_OK(hipMemcpy2DAsync(dst, row_bytes, pixels, (size_t)row_stride, row_bytes, (size_t)height, hipMemcpyHostToDevice, r.stream));
  return 0;
}

// the four Lanczos tables of one resize, appended to `coef`: kh | bh | kv | bv
struct ResizeTables { size_t off_kh = 0, off_bh = 0, off_kv = 0, off_bv = 0; int ksize_h = 0, ksize_v = 0; };
ResizeTables resize_tables(int w, int h, int out_w, int out_h, std::vector<int32_t> &coef) {
  ResizeTables t;
  std::vector<int32_t> kh, bh, kv, bv;
  t.ksize_h = lanczos_coeffs(w, out_w, kh, bh);
  t.ksize_v = lanczos_coeffs(h, out_h, kv, bv);
  const auto put = [&](const std::vector<int32_t> &v) { const size_t at = coef.size(); coef.insert(coef.end(), v.begin(), v.end()); return at; };
  t.off_kh = put(kh); t.off_bh = put(bh); t.off_kv = put(kv); t.off_bv = put(bv);
  return t;
}
// the six table fields of a launch-argument struct, from the tables' base in HBM and their offsets (ResizeTables, WindowGroup)
template <class Job, class Offsets>
void set_tables(Job &j, const int32_t *base, const Offsets &t) {
  j.kh = base + t.off_kh; j.bh = base + t.off_bh; j.ksize_h = t.ksize_h;
  j.kv = base + t.off_kv; j.bv = base + t.off_bv; j.ksize_v = t.ksize_v;
}

// The end of a device-pointer call's use of the shared workspaces, marked on the caller's stream `s` -- on a failing exit
// (rc != 0) too: passes queued before the failure still run.  Not while the stream is being captured into a graph: a
// replayed graph is serialised by its own stream, and the caller must not replay it concurrently with other calls into
// this library (include/bnn_mi355x.h).  Returns rc, or -1 when the mark itself failed.
int hand_over(const char *what, hipStream_t s, hipStreamCaptureStatus capturing, int rc) {
  Runtime &r = rt();
  if (s == r.stream || capturing != hipStreamCaptureStatusNone) return rc;
  const std::string why = r.err;
  if (hipEventRecord(r.ws_event, s) == hipSuccess) {
    r.ws_last = s;
    r.ws_pending = true;
    r.ws_gen++;
  } else if (rc == 0) {
    return fail(std::string(what) + ": recording the workspace hand-over failed");
  }
  if (rc) r.err = why;
  return rc;
}

// the result buffers of a pass of n images that bnn_mi355x_inference_device runs on records already in HBM
int reserve_results(size_t n) { return reserve_host(rt().stage_cap > 0 ? rt().stage_cap : 1, n); }

// the array an `int *` entry point returns (delete[]); null with last_error set
int *new_result(size_t count) {
  int *result = new (std::nothrow) int[count ? count : 1];
  if (!result) fail("out of memory");
  return result;
}

// The CNV results' way back on s (r.stream when none is given): the classes of n images straight into `result`, or -- `scores` sized by the
// caller to n x 64 -- the scores, which widen_scores puts into `result` as number_class ints per image after the sync
int enqueue_cnv_results(size_t n, int *result, std::vector<int16_t> &scores, hipStream_t s) {
  Runtime &r = rt();
  if (!scores.empty()) HIP_OK(hipMemcpyAsync(scores.data(), r.d_scores, n * 64 * sizeof(int16_t), hipMemcpyDeviceToHost, s));
  else HIP_OK(hipMemcpyAsync(result, r.d_classes, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  return 0;
}
int enqueue_cnv_results(size_t n, int *result, std::vector<int16_t> &scores) { return enqueue_cnv_results(n, result, scores, rt().stream); }
void widen_scores(const std::vector<int16_t> &scores, int number_class, int *result) {
  for (size_t i = 0; i < scores.size() / 64; i++)
    for (int j = 0; j < number_class; j++) result[i * number_class + j] = scores[i * 64 + j];
}

// The n records at r.d_gl_rec to classes (LFC), on r.stream: the pass bnn_mi355x_inference_device enqueues on records that
// never left the device, between gl_ev[1] and gl_ev[2]; the results' way back; the wait.  Up to 47 classes the last stage
// decodes on the device; beyond, the words come back and libm decodes them, as the reference does
// (bnn_mi355x_inference_device).  A status-2 glyph reads -1: its record was never written.  `status` may be null.
int classify_glyph_records(int n, int number_class, const std::vector<int32_t> &glyph_status, int *result, int *status) {
  Runtime &r = rt();
  const bool on_device = number_class <= 47;
  std::vector<uint64_t> words(on_device ? 0 : (size_t)n);
  HIP_OK(hipEventRecord(r.gl_ev[1], r.stream));
  if (bnn_mi355x_inference_device(r.d_gl_rec, n, number_class, on_device ? r.d_classes : nullptr, nullptr, r.d_words, r.stream)) return -1;
  HIP_OK(hipEventRecord(r.gl_ev[2], r.stream));
  if (on_device) HIP_OK(hipMemcpyAsync(result, r.d_classes, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
  else HIP_OK(hipMemcpyAsync(words.data(), r.d_words, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  for (int i = 0; i < n; i++) {
    if (!on_device) result[i] = lfc_class_batched(words[(size_t)i], number_class);
    if (glyph_status[(size_t)i] == kGlyphTooThin) result[i] = -1;
    if (status) status[i] = glyph_status[(size_t)i];
  }
  return 0;
}

// The n records at r.d_gl_rec to the caller's `records`, and the wait: a status-2 glyph's record stays as the caller left it
int download_glyph_records(size_t n, const std::vector<int32_t> &glyph_status, uint8_t *records, int *status) {
  Runtime &r = rt();
  std::vector<uint8_t> staged(n * kGlyphRecord);
  if (n) HIP_OK(hipMemcpyAsync(staged.data(), r.d_gl_rec, staged.size(), hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  for (size_t i = 0; i < n; i++) {
    if (glyph_status[i] != kGlyphTooThin) std::memcpy(records + i * kGlyphRecord, staged.data() + i * kGlyphRecord, kGlyphRecord);
    if (status) status[i] = glyph_status[i];
  }
  return 0;
}

}  // namespace
}  // namespace bnn

#ifdef BNN_LFC_STAMPS
namespace bnn { hipError_t lfc_stamps_read(unsigned long long *dst); hipError_t lfc_wstamps_read(unsigned long long *dst); }
#endif
using namespace bnn;

// ============================================================================ C ABI
extern "C" {

void load_parameters(const char *path) {
  Runtime &r = rt();
  std::printf("Setting network weights and thresholds in accelerator...\n");
  RawParams raw;
  const std::string e = read_raw_params(r.spec, path ? path : "", raw);
  if (!e.empty()) { fail(e); return; }
  r.raw = std::move(raw);
  pack_blob(r.spec, r.raw, r.blob);
  if (upload_blob()) { r.blob.clear(); return; }
  r.err.clear();
  (void)warm_up();  // failure is reported (stderr, last_error) but the parameters are loaded
}

int inference(const char *path, int results[64], int number_class, float *usecPerImage) {
  Runtime &r = rt();
  if (!ready()) return -1;
  ImageFile f;
  trace().start();
  if (open_image_file(path, f)) return -1;
  trace().mark("opened");
  if (f.n == 0) return fail("no image in input file");
  float usec = 0.f;
  int cls;
  if (r.spec.is_cnv) {
    // testPrebuiltCIFAR10_from_image: count = 1 (foldedmv-offload.h:318): the first record of the file
    int16_t s[64];
    if (infer_file(f, 1, number_class, nullptr, s, nullptr, &usec)) return -1;
    if (results)
      for (int j = 0; j < number_class; j++) results[j] = s[j];
    cls = 0;
    for (int j = 1; j < number_class; j++)
      if (s[j] > s[cls]) cls = j;  // std::max_element: first maximum
  } else {
    uint64_t w = 0;
    if (infer_file(f, 1, number_class, nullptr, nullptr, &w, &usec)) return -1;
    const int hot = lfc_hot_single(w, number_class);
    if (results)
      for (int i = 0; i < 64; i++) results[i] = (i == hot) ? 1 : 0;
    cls = hot < 64 ? hot : 0;
  }
  std::printf("Inference took %.0f microseconds, %g usec per image\n", usec, usec);
  std::printf("Classification rate: %g images per second\n", 1000000.0 / usec);
  if (usecPerImage) *usecPerImage = usec;
  return cls;
}

int *inference_multiple(const char *path, int number_class, int *image_number, float *usecPerImage,
                        int enable_detail) {
  if (!ready()) return nullptr;
  ImageFile f;
  trace().start();
  if (open_image_file(path, f)) return nullptr;
  trace().mark("opened");
  const int n = (int)f.n;
  float usec = 0.f;
  int *res = classify_with([&](int32_t *c, int16_t *s, uint64_t *w, const uint64_t **v) { return infer_file(f, n, number_class, c, s, w, &usec, v); }, n,
                           number_class, enable_detail);
  if (!res) return nullptr;
  std::printf("Inference took %.0f microseconds, %g usec per image\n", usec * n, usec);
  std::printf("Classification rate: %g images per second\n", 1000000.0 / usec);
  if (image_number) *image_number = n;
  if (usecPerImage) *usecPerImage = usec;
  return res;
}

int *inference_multiple_with_faults(const char *path, int number_class, int *image_number,
                                    float *usecPerImage, unsigned int flip_count, int word_size,
                                    int target, int *target_layers, unsigned int num_targets) {
  Runtime &r = rt();
  if (flip_count == 0) return inference_multiple(path, number_class, image_number, usecPerImage, 0);
#ifdef BNN_VARIANT
  // TMRBinaryWeights / the interleaved memories live in the un-vendored finn-hlslib fork: their voting
  // and de-interleaving are not restated here, so a fault campaign would not mean what the caller expects
  fail("fault injection is not modelled for " BNN_VARIANT " (replicated / interleaved parameter memories); use the base network");
  return nullptr;
#endif
  if (!ready()) return nullptr;
  if (r.raw.empty()) {
    fail("fault injection needs the parameter files (load_parameters), not an imported blob");
    return nullptr;
  }
  if (r.l1_mfma || r.l1_literal) {
    fail("fault injection is not wired to the BNN_MI355X_L1 comparison forms (the matrix-pipe table is not patched)");
    return nullptr;
  }
  ImageFile f;
  if (open_image_file(path, f)) return nullptr;
  const int n = (int)f.n;
  // The reference classifies image by image and injects each fault just before the image it was
  // drawn for (faults.h:115-148).  Same result, fewer launches: the images go to HBM once, the run
  // of images between two fault times is classified as one batch, and a fault patches the one
  // affected row of the blob in HBM -- all of it queued on one stream, one wait at the end.
  {
    const std::string pe = plan_faults(r.spec, r.fault_seed, n, flip_count, word_size, target, target_layers, num_targets, r.last_faults);
    if (!pe.empty()) { fail(pe); return nullptr; }
  }
  int *result = new (std::nothrow) int[(size_t)(n > 0 ? n : 1)];
  if (!result) { fail("out of memory"); return nullptr; }
  auto run = [&]() -> int {
    if (n == 0) return 0;
    const size_t isz = (size_t)r.spec.image_bytes();
    if (load_file_resident(f, n)) return -1;
    if (reserve(n) || reserve_host(1, (size_t)n)) return -1;
    std::vector<std::vector<uint8_t>> patches;  // row images must outlive their asynchronous upload
    patches.reserve(r.last_faults.size());
    DrainOnFailure drain;  // (declared after `patches`: a failing return drains the stream before they are released)
    // one pair of events around the whole campaign: the row patches between the runs are a few hundred
    // bytes each, and an event pair per run would cost more than they do
    while (r.time_events.size() < 2) {
      hipEvent_t e;
      HIP_OK(hipEventCreateWithFlags(&e, kTimeEventFlags));
      r.time_events.push_back(e);
    }
    HIP_OK(hipEventRecord(r.time_events[0], r.stream));
    size_t k = 0;
    int start = 0;
    while (start < n) {
      while (k < r.last_faults.size() && r.last_faults[k].image <= start) {
        const Fault &flt = r.last_faults[k++];
        const int row = apply_fault(r.spec, r.raw, flt);
        if (row < 0) continue;
        size_t off = 0, bytes = 0;
        repack_row(r.spec, r.raw, flt.layer, row, r.blob, &off, &bytes);
        if (r.spec.L[flt.layer].arith == AR_TT) r.two_rows = count_two_rows(r.spec, r.blob);
        patches.emplace_back(r.blob.begin() + off, r.blob.begin() + off + bytes);
        HIP_OK(hipMemcpyAsync(static_cast<uint8_t *>(r.d_blob) + off, patches.back().data(), bytes, hipMemcpyHostToDevice, r.stream));
      }
      const int end = (k < r.last_faults.size()) ? r.last_faults[k].image : n;
      for (int base = start; base < end; base += kMaxChunk) {
        const int m = (end - base < kMaxChunk) ? end - base : kMaxChunk;
        if (enqueue(r.d_all + (size_t)base * isz, m, number_class, r.d_classes + base, nullptr, r.d_words + base, r.stream)) return -1;
      }
      start = end;
    }
    HIP_OK(hipEventRecord(r.time_events[1], r.stream));
    std::vector<uint64_t> w;
    if (r.spec.is_cnv) {
      HIP_OK(hipMemcpyAsync(result, r.d_classes, (size_t)n * 4, hipMemcpyDeviceToHost, r.stream));
    } else {  // host decode, like the batched LFC entry point
      w.resize((size_t)n);
      HIP_OK(hipMemcpyAsync(w.data(), r.d_words, (size_t)n * 8, hipMemcpyDeviceToHost, r.stream));
    }
    HIP_OK(hipStreamSynchronize(r.stream));
    for (int i = 0; !r.spec.is_cnv && i < n; i++) result[i] = lfc_class_batched(w[i], number_class);
    float ms_total = 0.f;
    HIP_OK(hipEventElapsedTime(&ms_total, r.time_events[0], r.time_events[1]));
    drain.ok();
    return (int)(ms_total * 1000.0 + 0.5);  // device microseconds of the campaign
  };
  // The campaign runs the XNOR-popcount kernels (its row patches land between the batches, the matrix forms' tables are
  // made from the rows once); the patches persist, so the tables are remade from the patched rows behind them.
  r.conv_xnor = true;
  const int total_us = run();
  r.conv_xnor = false;
  if (make_conv_tables(r.stream) || total_us < 0) {
    delete[] result;
    return nullptr;
  }
  const float usec = n > 0 ? (float)total_us / (float)n : 0.f;
  std::printf("Inference took %.0f microseconds, %g usec per image\n", (double)total_us, usec);
  std::printf("Classification rate: %g images per second\n", 1000000.0 / usec);
  if (image_number) *image_number = n;
  if (usecPerImage) *usecPerImage = usec;
  return result;
}

int *bnn_mi355x_fault_campaigns(const char *path, int number_class, int num_runs, unsigned long long seed,
                                unsigned int flip_count, int word_size, int target, const int *target_layers,
                                unsigned int num_targets, int *image_number, float *usecPerImage) {
  Runtime &r = rt();
  r.camp_faults.clear();
  r.camp_run.clear();
  if (num_runs < 1 || num_runs > kMaxRuns) {
    fail("fault_campaigns: num_runs must be 1 ... " + std::to_string(kMaxRuns));
    return nullptr;
  }
  const int R = num_runs;
  // run q seeds with seed + q: none of them may be 0, which would mean std::random_device
  if (seed != 0 && 0ull - (uint64_t)seed < (uint64_t)R) {
    fail("fault_campaigns: seed + run wraps to 0 for a run (0 seeds from std::random_device)");
    return nullptr;
  }
  if (flip_count == 0) {  // like inference_multiple_with_faults: the fault-free classes, once per run
    int n = 0;
    float usec = 0.f;
    int *one = inference_multiple(path, number_class, &n, &usec, 0);
    if (!one) return nullptr;
    int *res = new (std::nothrow) int[(size_t)R * n + 1];
    if (!res) { free_results(one); fail("out of memory"); return nullptr; }
    for (int q = 0; q < R; q++) std::memcpy(res + (size_t)q * n, one, (size_t)n * sizeof(int));
    free_results(one);
    if (image_number) *image_number = n;
    if (usecPerImage) *usecPerImage = usec / (float)R;
    return res;
  }
#ifdef BNN_VARIANT
  fail("fault injection is not modelled for " BNN_VARIANT " (replicated / interleaved parameter memories); use the base network");
  return nullptr;
#endif
  if (!ready()) return nullptr;
  if (r.raw.empty()) {
    fail("fault injection needs the parameter files (load_parameters), not an imported blob");
    return nullptr;
  }
  if (r.l1_mfma || r.l1_literal) {
    fail("fault injection is not wired to the BNN_MI355X_L1 comparison forms (the matrix-pipe table is not patched)");
    return nullptr;
  }
  ImageFile f;
  if (open_image_file(path, f)) return nullptr;
  const int n = (int)f.n;
  const size_t total = (size_t)R * n;
  // every run's plan, drawn exactly as inference_multiple_with_faults draws it with the fault seed set to seed + q
  std::vector<Fault> faults;
  std::vector<int> run_of;
  for (int q = 0; q < R; q++) {
    std::vector<Fault> plan;
    const std::string pe = plan_faults(r.spec, seed ? (uint64_t)seed + (uint64_t)q : 0, n, flip_count, word_size, target, target_layers,
                                       num_targets, plan);
    if (!pe.empty()) { fail(pe); return nullptr; }
    faults.insert(faults.end(), plan.begin(), plan.end());
    run_of.insert(run_of.end(), plan.size(), q);
  }
  int *result = new (std::nothrow) int[total + 1];
  if (!result) { fail("out of memory"); return nullptr; }
  const int F = (int)flip_count;  // (n > 0: every run has exactly F faults, sorted by image)
  double device_us = 0.0;
  auto run = [&]() -> int {
    if (n == 0) return 0;
    if (faults.size() != (size_t)R * F) return fail("internal: fault plans of unequal length");
    // -- host: the patches.  ONE working copy of the memories and the blob; each run's faults are applied in order, every
    // rebuilt row recorded as that fault's patch, then undone (the touched words restored, the touched rows rebuilt).
    RawParams raw = r.raw;
    std::vector<uint8_t> blob = r.blob;
    PackedHeader h;
    std::memcpy(&h, blob.data(), sizeof(h));
    const size_t stride = (blob.size() + 255) & ~(size_t)255;
    const bool tab = h.l0_mfma_offset && r.l0_mfma;  // layer-0 faults patch the MFMA table too (kernels read it)
    std::vector<uint8_t> staging;
    std::vector<std::vector<PatchSpan>> by_wave((size_t)F + 1);  // wave k (>= 1): the k-th patch of every run
    std::vector<char> wave_two((size_t)F + 1, 0);                // wave k: some run's copy holds a -2 row (cnvW2A2)
    auto two_flag = [&](int l, int row) -> int {
      if (r.spec.L[l].arith != AR_TT) return 0;
      const uint32_t *rows = reinterpret_cast<const uint32_t *>(blob.data() + h.layer[l].offset);
      return rows[(size_t)row * h.layer[l].row_dwords + 2 + 6 * h.layer[l].kw] != 0;
    };
    auto add_span = [&](int k, int q, size_t off, size_t bytes) {
      by_wave[(size_t)k].push_back(PatchSpan{(uint64_t)q * stride + off, (uint32_t)staging.size(), (uint32_t)bytes});
      staging.insert(staging.end(), blob.begin() + off, blob.begin() + off + bytes);
    };
    const int base_two = count_two_rows(r.spec, blob);  // (once: per fault the count follows the patched row)
    struct Saved { uint64_t *word; uint64_t old; };
    std::vector<Saved> saved;
    std::vector<std::pair<int, int>> touched;
    for (int q = 0; q < R; q++) {
      int two = base_two;
      if (two > 0) wave_two[0] = 1;
      saved.clear();
      touched.clear();
      for (int k = 0; k < F; k++) {
        const Fault &flt = faults[(size_t)q * F + k];
        if (uint64_t *w = fault_word(r.spec, raw, flt)) {
          saved.push_back({w, *w});
          const int row = apply_fault(r.spec, raw, flt);
          const int before = two_flag(flt.layer, row);
          size_t off = 0, bytes = 0;
          repack_row(r.spec, raw, flt.layer, row, blob, &off, &bytes);
          touched.emplace_back(flt.layer, row);
          two += two_flag(flt.layer, row) - before;
          if (flt.layer == 0 && h.l0_mfma_offset) {  // repack_row's span runs from the row to the table's end: the two parts
            const size_t rb = (size_t)h.layer[0].row_dwords * 4;
            add_span(k + 1, q, h.layer[0].offset + (size_t)row * rb, rb);
            if (tab) add_span(k + 1, q, h.l0_mfma_offset, kL0MfmaBytes);
          } else {
            add_span(k + 1, q, off, bytes);
          }
        }
        if (two > 0) wave_two[(size_t)k + 1] = 1;
      }
      for (size_t i = saved.size(); i-- > 0;) *saved[i].word = saved[i].old;
      for (auto &t : touched) {
        size_t off, bytes;
        repack_row(r.spec, raw, t.first, t.second, blob, &off, &bytes);
      }
    }
    if (staging.size() > 0xFFFFFFF0u) return fail("fault_campaigns: too many faults for one call (patch staging above 4 GB)");
    // -- segments: wave k classifies, for every run, the images between its k-th and (k+1)-th fault time.  A launch holds
    // at most `cap` images (the activation workspace) and 65 535 records (grid.y); a longer wave is cut over several.
    const int cap = (int)std::min<size_t>(kMaxChunk, total);
    struct Launch { size_t seg0; int nsegs, max_len, total, wave; };
    std::vector<MultiSeg> segs;
    std::vector<Launch> launches;
    for (int k = 0; k <= F; k++) {
      Launch cur{segs.size(), 0, 0, 0, k};
      auto close = [&]() {
        if (cur.nsegs) launches.push_back(cur);
        cur = Launch{segs.size(), 0, 0, 0, k};
      };
      for (int q = 0; q < R; q++) {
        int b = k ? faults[(size_t)q * F + k - 1].image : 0;
        const int e = k < F ? faults[(size_t)q * F + k].image : n;
        while (b < e) {
          if (cur.total == cap || cur.nsegs == 65535) close();
          const int m = std::min(e - b, cap - cur.total);
          segs.push_back(MultiSeg{q, b, cur.total, m});
          cur.nsegs++;
          cur.total += m;
          cur.max_len = std::max(cur.max_len, m);
          b += m;
        }
      }
      close();
    }
    // -- one upload: patches, then patch spans by wave, then segment records
    std::vector<size_t> span_first((size_t)F + 2, 0);
    for (int k = 0; k <= F; k++) span_first[(size_t)k + 1] = span_first[(size_t)k] + by_wave[(size_t)k].size();
    const size_t spans_off = (staging.size() + 255) & ~(size_t)255;
    const size_t segs_off = spans_off + span_first[(size_t)F + 1] * sizeof(PatchSpan);
    std::vector<uint8_t> upload(segs_off + segs.size() * sizeof(MultiSeg));
    std::memcpy(upload.data(), staging.data(), staging.size());
    for (int k = 0; k <= F; k++)
      if (!by_wave[(size_t)k].empty())
        std::memcpy(upload.data() + spans_off + span_first[(size_t)k] * sizeof(PatchSpan), by_wave[(size_t)k].data(), by_wave[(size_t)k].size() * sizeof(PatchSpan));
    if (!segs.empty()) std::memcpy(upload.data() + segs_off, segs.data(), segs.size() * sizeof(MultiSeg));
    // -- device buffers
    const bool cnv = r.spec.is_cnv;
    if (load_file_resident(f, n) || reserve(cap)) return -1;
    if (r.d_copies.grow((size_t)R * stride) || r.d_camp.grow(upload.size()) ||
        r.d_camp_res.grow(total * (cnv ? sizeof(int32_t) : sizeof(uint64_t))))
      return -1;
    std::vector<uint64_t> w;  // (LFC: raw words, decoded on the host)
    if (!cnv) w.resize(total);
    DrainOnFailure drain;  // (declared after the host buffers the queued copies read or write)
    if (settle_handover(r.stream)) return -1;
    while (r.time_events.size() < 2) {
      hipEvent_t e;
      HIP_OK(hipEventCreateWithFlags(&e, kTimeEventFlags));
      r.time_events.push_back(e);
    }
    // -- all of it on one stream, one wait at the end
    HIP_OK(hipEventRecord(r.time_events[0], r.stream));
    HIP_OK(hipMemcpyAsync(r.d_copies, r.d_blob, blob.size(), hipMemcpyDeviceToDevice, r.stream));
    for (size_t have = 1; have < (size_t)R; have *= 2) {  // replicate by doubling
      const size_t c = std::min(have, (size_t)R - have);
      HIP_OK(hipMemcpyAsync(r.d_copies + have * stride, r.d_copies, c * stride, hipMemcpyDeviceToDevice, r.stream));
    }
    HIP_OK(hipMemcpyAsync(r.d_camp, upload.data(), upload.size(), hipMemcpyHostToDevice, r.stream));
    const PatchSpan *d_spans = reinterpret_cast<const PatchSpan *>(r.d_camp + spans_off);
    const MultiSeg *d_segs = reinterpret_cast<const MultiSeg *>(r.d_camp + segs_off);
    size_t li = 0;
    for (int k = 0; k <= F; k++) {
      const int ns = (int)(span_first[(size_t)k + 1] - span_first[(size_t)k]);
      hipError_t e = scatter_patches(r.d_camp, d_spans + span_first[(size_t)k], ns, r.d_copies, r.stream);
      if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
      for (; li < launches.size() && launches[li].wave == k; li++) {
        const Launch &L = launches[li];
        MultiLaunch a{};
        a.images = r.d_all;
        a.segs = d_segs + L.seg0;
        a.nsegs = L.nsegs; a.max_len = L.max_len; a.total = L.total; a.n = n;
        a.buf0 = r.buf0; a.buf1 = r.buf1;
        for (int l = 0; l < r.spec.nlayers; l++) a.rows[l] = reinterpret_cast<const uint32_t *>(r.d_copies + h.layer[l].offset);
        a.l0_mfma = tab ? r.d_copies + h.l0_mfma_offset : nullptr;
        a.stride = stride;
        a.has_two = wave_two[(size_t)k] != 0;
        a.classes = reinterpret_cast<int32_t *>(r.d_camp_res.get());
        a.words = reinterpret_cast<uint64_t *>(r.d_camp_res.get());
        a.number_class = number_class;
        a.stream = r.stream;
        e = cnv ? run_cnv_multi(r.spec.id, a) : run_lfc_multi(r.spec.id, a);
        if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
      }
    }
    HIP_OK(hipEventRecord(r.time_events[1], r.stream));
    if (cnv) HIP_OK(hipMemcpyAsync(result, r.d_camp_res, total * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
    else HIP_OK(hipMemcpyAsync(w.data(), r.d_camp_res, total * sizeof(uint64_t), hipMemcpyDeviceToHost, r.stream));
    HIP_OK(hipStreamSynchronize(r.stream));
    for (size_t i = 0; !cnv && i < total; i++) result[i] = lfc_class_batched(w[i], number_class);
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, r.time_events[0], r.time_events[1]));
    drain.ok();
    device_us = ms * 1000.0;
    return 0;
  };
  if (run() < 0) {
    delete[] result;
    return nullptr;
  }
  r.camp_faults = std::move(faults);
  r.camp_run = std::move(run_of);
  if (image_number) *image_number = n;
  if (usecPerImage) *usecPerImage = total ? (float)(device_us / (double)total) : 0.f;
  return result;
}

// The fault records of the C ABI: 8 ints {image, target, layer, mem, ind, thresh, bit, word_size}; a physical fault's
// (mem_org.h) have the module as a ninth.
static void put_record(const Fault &f, int *w) {
  const int v[8] = {f.image, f.target, f.layer, f.mem, f.ind, f.thresh, f.bit, f.word_size};
  std::memcpy(w, v, sizeof v);
}
static void put_record(const PhysFault &pf, int *w) {
  put_record(pf.f, w);
  w[8] = pf.module;
}
static Fault fault_record(const int *v) { return Fault{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]}; }
static PhysFault phys_fault_record(const int *v) { return PhysFault{fault_record(v), v[8]}; }

// the tail of every pack_params_* entry point: the memories packed as load_parameters packs them, copied out where dst is given
static size_t pack_params_out(const std::string &who, const RawParams &raw, void *dst, size_t cap) {
  std::vector<uint8_t> blob;
  pack_blob(rt().spec, raw, blob);
  if (dst) {
    if (cap < blob.size()) { fail(who + ": destination too small"); return 0; }
    std::memcpy(dst, blob.data(), blob.size());
  }
  return blob.size();
}

int bnn_mi355x_last_campaign_faults(int *records, int cap_records) {
  Runtime &r = rt();
  const int n = (int)r.camp_faults.size();
  for (int i = 0; i < n && i < cap_records && records; i++) {
    records[i * 9] = r.camp_run[(size_t)i];
    put_record(r.camp_faults[(size_t)i], records + i * 9 + 1);
  }
  return n;
}

long bnn_mi355x_enumerate_faults(int layer, int target, int word_size, long first, int *records, int cap_records) {
  const NetSpec &net = rt().spec;
  const long total = enumerate_faults(net, layer, target, word_size, 0, nullptr, 0);
  if (total < 0 || first < 0) return fail("enumerate_faults: bad layer, target (0 weights, 1 thresholds), word_size (1 ... 64) or first");
  if (records && cap_records > 0 && first < total) {
    std::vector<Fault> v((size_t)std::min<long>(cap_records, total - first));
    enumerate_faults(net, layer, target, word_size, first, v.data(), (long)v.size());
    for (size_t i = 0; i < v.size(); i++) put_record(v[i], records + i * 8);
  }
  return total;
}

// A sweep that runs with profiling on replaces the last profile: none is left if it fails (bnn_mi355x_last_sweep_profile).
static void sweep_profile_begin(Runtime &r) {
  if (!r.sweep_profile) return;
  r.prof_alive.clear();
  r.prof_flipped.clear();
  r.prof_rows = 0;
  r.prof_cols = 0;
}

// The body the single-fault sweeps share, behind their entry points' checks: bnn_mi355x_fault_sweep (parameter faults,
// `faults`), bnn_mi355x_act_fault_sweep (activation sites, `sites`) and bnn_mi355x_input_fault_sweep (bits of the image
// buffer, `inputs`: a site "layer" before layer 0); the other two are null.  A group of records in
// layer L starts at stage s0: a parameter fault at L itself, from blob copies patched for the group and the broadcast
// fault-free output of layer L-1; an activation site at L+1, from the loaded blob (copy stride 0) and k_act_seed's rows --
// or, for the CNV site layers 0..2, with layer L+1 evaluated only inside the window the site reaches (act_window: the
// fault-free layer-(L+1) rows broadcast, the window's pixels recomputed over them; no faulted layer-L row is written).
// An input site starts at layer 0 (LFC: its binariser) like a layer-0 parameter fault, but from k_input_seed's faulted
// copies of the images in a staging buffer and the loaded blob: layer 0's records then name the staged slot as their image.
// The per-layer pair counts go to `stage_pairs` on success.
static long single_fault_sweep(const char *path, int number_class, const std::vector<Fault> *faults, const std::vector<ActSite> *sites,
                               const std::vector<InputSite> *inputs, int *changed, int *diffs, long cap_diffs, int *image_number,
                               float *usecPerImage, std::vector<long> &stage_pairs) {
  Runtime &r = rt();
  const NetSpec &net = r.spec;
  const bool act = sites != nullptr, inp = inputs != nullptr;
  const bool unpatched = act || inp;  // (neither patches a parameter: the loaded blob, copy stride 0, no group bound by kMaxRuns)
  const int n_faults = (int)(inp ? inputs->size() : act ? sites->size() : faults->size());
  const auto layer_of = [&](int i) { return inp ? 0 : act ? (*sites)[(size_t)i].layer : (*faults)[(size_t)i].layer; };
  const auto start_of = [&](int L) { return act ? L + 1 : L; };
  ImageFile f;
  if (open_image_file(path, f)) return -1;
  const int n = (int)f.n, S = net.nlayers;
  const bool cnv = net.is_cnv;
  std::vector<long> pairs((size_t)S, 0);
  // the propagation profile (bnn_mi355x_sweep_profile): per record and layer with an output map, the images and the
  // activations that differ from the fault-free output
  const bool profile = r.sweep_profile;
  std::vector<long> prof_alive(profile ? (size_t)n_faults * (size_t)(S - 1) : 0, 0), prof_flipped(prof_alive.size(), 0);
  if (n_faults) std::fill(changed, changed + n_faults, 0);
  long total_changed = 0;
  double device_us = 0.0;
  // the first cap_diffs diffs in (fault, image) order: per fault its {image, class} pairs; a fault's list is dropped
  // once the lists of the faults before it hold cap_diffs pairs
  std::map<int, std::vector<int>> kept;
  long kept_n = 0;
  auto keep = [&](int fi, const int *pv, long cnt) {
    if (cap_diffs == 0 || cnt == 0) return;
    std::vector<int> &d = kept[fi];
    d.insert(d.end(), pv, pv + 2 * cnt);
    kept_n += cnt;
    while (!kept.empty() && kept_n - (long)(kept.rbegin()->second.size() / 2) >= cap_diffs) {
      kept_n -= (long)(kept.rbegin()->second.size() / 2);
      kept.erase(std::prev(kept.end()));
    }
  };
  auto run = [&]() -> int {
    if (n == 0 || n_faults == 0) return 0;
    // -- geometry.  Layer l < S-1 leaves `ob[l]` bytes per image in buffer `obuf[l]` (stage_output_bytes); the fault-free
    // outputs of all n images are kept at base + boff[l], the fault-free results (class / raw word, rb bytes) behind them.
    std::vector<size_t> ob((size_t)S, 0), boff((size_t)S + 1, 0);
    std::vector<int> obuf((size_t)S, 0);
    const std::vector<int> ipi = cnv ? std::vector<int>{900, 196, 36, 25, 9, 1, 1, 1, 1} : std::vector<int>{1, 1, 1, 1};  // work items per image
    const size_t rb = cnv ? sizeof(int32_t) : sizeof(uint64_t);
    for (int l = 0; l < S; l++) {
      if (l + 1 < S) ob[(size_t)l] = stage_output_bytes(cnv, net.abits, cnv ? l : l + 1, &obuf[(size_t)l]);
      boff[(size_t)l + 1] = boff[(size_t)l] + (((l + 1 < S ? ob[(size_t)l] : rb) * (size_t)n + 255) & ~(size_t)255);
    }
    size_t b0, b1;
    if (cnv) cnv_workspace_bytes(net.abits, &b0, &b1);
    else lfc_workspace_bytes(net.abits, &b0, &b1);
    const int wcap = (int)std::min<long long>(kMaxChunk, (long long)n_faults * n);  // images of activation workspace
    // activation sites (read at every call): BNN_MI355X_ACT_WINDOW=0 keeps the dense first stage for every layer, any other
    // value takes the windowed one for every CNV site layer 0..2 (the A/B switch, and the tests' two routes); unset, the
    // policy below decides.  BNN_MI355X_SWEEP_GROUP=<pairs> caps a run group's pairs (tests: several groups and image
    // windows on few images).
    // Policy: per (net, site layer) the windowed route only where a record of tools/act_fault_sweep_rate.py --window-ab has
    // it faster than the dense one by more than the spread between repeats.  No such record yet: every case stays dense.
    static const bool kWindowFaster[3][3] = {{false, false, false}, {false, false, false}, {false, false, false}};
    const char *const env_win = std::getenv("BNN_MI355X_ACT_WINDOW");
    const auto windowed = [&](int L) {
      if (!act || !cnv || L > 2) return false;
      return env_win ? std::atoi(env_win) != 0 : kWindowFaster[net.id][L];
    };
    long long group_cap = 0;
    if (const char *e = unpatched ? std::getenv("BNN_MI355X_SWEEP_GROUP") : nullptr) group_cap = std::atoll(e);
    // A run group that starts at stage s0 holds the outputs of layers s0-1 .. S-2 in the workspace at once, (run, image)
    // slot by slot: its pairs are bounded by the bytes per image of those outputs, not by the layer-0 sizing of the
    // workspace -- the FC layers take ~25x the pairs of the conv layers.  Activation sites need no blob copies: their
    // groups are not bounded by kMaxRuns; a windowed group never holds layer s0-1's output either.
    std::vector<int> G((size_t)S, 0), win((size_t)S, 0);
    std::vector<std::vector<int>> by_layer((size_t)S);
    for (int i = 0; i < n_faults; i++) by_layer[(size_t)layer_of(i)].push_back(i);
    long long max_pairs = 0;
    int max_runs = 0;
    for (int L = 0; L < S; L++) {
      if (by_layer[(size_t)L].empty()) continue;
      const int s0 = start_of(L);
      long long c = kMaxSweepPairs;
      for (int l = windowed(L) ? s0 : std::max(s0 - 1, 0); l + 1 < S; l++)
        c = std::min<long long>(c, (long long)((size_t)wcap * (obuf[(size_t)l] ? b1 : b0) / ob[(size_t)l]));
      if (s0 == 0) c = std::min<long long>(c, wcap);  // (the first stage writes the layer-0 sizes)
      if (inp) c = std::min<long long>(c, kInputStagePairs);  // (the staged images)
      if (group_cap > 0) c = std::min(c, group_cap);
      const long long runs_cap = unpatched ? kMaxSweepPairs : (long long)kMaxRuns;
      const int g = (int)std::max<long long>(1, std::min<long long>({c / n, runs_cap, (long long)by_layer[(size_t)L].size()}));
      G[(size_t)L] = g;
      win[(size_t)L] = g > 1 ? n : (int)std::min<long long>(n, c);
      max_pairs = std::max(max_pairs, (long long)g * win[(size_t)L]);
      max_runs = std::max(max_runs, g);
    }
    // -- host: the working copy of the memories and the blob that patches are built on (restored after every fault)
    RawParams raw = unpatched ? RawParams{} : r.raw;  // (activation and input sites patch nothing)
    std::vector<uint8_t> blob = r.blob;
    PackedHeader h;
    std::memcpy(&h, blob.data(), sizeof(h));
    const size_t stride = (blob.size() + 255) & ~(size_t)255;
    const bool tab = h.l0_mfma_offset && r.l0_mfma;  // layer-0 faults patch the MFMA table too (kernels read it)
    const int base_two = count_two_rows(net, r.blob);
    auto two_flag = [&](int l, int row) -> int {
      if (net.L[l].arith != AR_TT) return 0;
      const uint32_t *rows = reinterpret_cast<const uint32_t *>(blob.data() + h.layer[l].offset);
      return rows[(size_t)row * h.layer[l].row_dwords + 2 + 6 * h.layer[l].kw] != 0;
    };
    // -- device buffers
    const size_t res_n = std::max<size_t>((size_t)max_pairs, (size_t)n);
    if (load_file_resident(f, n) || reserve(wcap)) return -1;
    const size_t isz = (size_t)net.image_bytes();
    if (r.d_copies.grow(unpatched ? 0 : (size_t)max_runs * stride) || r.d_sw_base.grow(boff[(size_t)S]) ||
        r.d_in_stage.grow(inp ? (size_t)max_pairs * isz + 256 : 0) ||
        r.d_sw_segs.grow((size_t)max_pairs * sizeof(MultiSeg) * (inp ? 2 : 1)) || r.d_sw_alive.grow((size_t)max_pairs) ||
        r.d_sw_res.grow(res_n * rb) || r.d_sw_cnt.grow((size_t)max_runs * 12 + 512) ||
        r.d_sw_diffs.grow((size_t)max_pairs * 8) || r.d_sw_prof.grow(profile ? (size_t)max_runs * 16 : 0))
      return -1;
    uint8_t *const bufs[2] = {static_cast<uint8_t *>(r.buf0), static_cast<uint8_t *>(r.buf1)};
    uint8_t *const base_res = r.d_sw_base + boff[(size_t)S - 1];
    int *const d_counts = reinterpret_cast<int *>(r.d_sw_cnt.get());
    long long *const d_offsets = reinterpret_cast<long long *>(r.d_sw_cnt + (((size_t)max_runs * 4 + 255) & ~(size_t)255));
    const MultiSeg *const d_segs = reinterpret_cast<const MultiSeg *>(r.d_sw_segs.get());
    MultiSeg *const d_seed_segs = reinterpret_cast<MultiSeg *>(r.d_sw_segs.get()) + max_pairs;  // (input sites: layer 0's records, below)
    // host buffers the queued copies read or write (declared before `drain`)
    std::vector<MultiSeg> segs, ran, seed_segs;
    std::vector<uint8_t> alive, upload;
    std::vector<unsigned long long> prof;
    std::vector<int> counts, pv;
    std::vector<long long> offs;
    std::vector<uint64_t> words;
    std::vector<int> base_cls((size_t)n);
    DrainOnFailure drain;
    if (settle_handover(r.stream)) return -1;
    while (r.time_events.size() < 2) {
      hipEvent_t e;
      HIP_OK(hipEventCreateWithFlags(&e, kTimeEventFlags));
      r.time_events.push_back(e);
    }
    // device time: the sum of the bursts of work between two host waits
    bool open = false;
    auto begin = [&]() -> int {
      if (!open) HIP_OK(hipEventRecord(r.time_events[0], r.stream));
      open = true;
      return 0;
    };
    auto finish = [&]() -> int {
      if (open) HIP_OK(hipEventRecord(r.time_events[1], r.stream));
      HIP_OK(hipStreamSynchronize(r.stream));
      if (open) {
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, r.time_events[0], r.time_events[1]));
        device_us += ms * 1000.0;
      }
      open = false;
      return 0;
    };
    // launches over `segs`: grouped by length class (grid.x follows a launch's longest record), at most 65 535 records each
    struct Batch { size_t seg0; int nsegs, max_len, total; };
    std::vector<Batch> batches;
    std::vector<MultiSeg> sorted;
    auto plan = [&]() -> int {
      batches.clear();
      size_t cnt[33] = {}, at[33] = {};
      auto cls = [](int len) { return 32 - __builtin_clz((unsigned)len); };
      for (const MultiSeg &sg : segs) cnt[cls(sg.len)]++;
      for (int c = 1; c < 33; c++) at[c] = at[c - 1] + cnt[c - 1];
      sorted.resize(segs.size());
      for (const MultiSeg &sg : segs) sorted[at[cls(sg.len)]++] = sg;
      segs.swap(sorted);
      for (size_t i = 0; i < segs.size();) {
        Batch b{i, 0, 0, 0};
        const int c = cls(segs[i].len);
        for (; i < segs.size() && cls(segs[i].len) == c && b.nsegs < 65535; i++) {
          b.nsegs++;
          b.total += segs[i].len;
          b.max_len = std::max(b.max_len, segs[i].len);
        }
        batches.push_back(b);
      }
      HIP_OK(hipMemcpyAsync(r.d_sw_segs, segs.data(), segs.size() * sizeof(MultiSeg), hipMemcpyHostToDevice, r.stream));
      return 0;
    };
    // layer l's stage over the batches: rows from `copies` (run q's copy at q * cstride), results to `res`
    // (`window`: the windowed first stage of an activation-site group instead, from the fault-free layer l-1 rows;
    // `staged`: layer 0 of an input-site group, its images the staged ones that the records of `staged_segs` name)
    auto stage = [&](int l, const uint8_t *copies, size_t cstride, bool two, uint8_t *res, const ActWinSite *window = nullptr,
                     const uint8_t *staged = nullptr, const MultiSeg *staged_segs = nullptr) -> int {
      for (const Batch &b : batches) {
        MultiLaunch a{};
        a.images = staged ? staged : r.d_all;
        a.segs = (staged ? staged_segs : d_segs) + b.seg0;
        a.nsegs = b.nsegs; a.max_len = b.max_len; a.total = b.total; a.n = n;
        a.buf0 = r.buf0; a.buf1 = r.buf1;
        for (int k = 0; k < S; k++) a.rows[k] = reinterpret_cast<const uint32_t *>(copies + h.layer[k].offset);
        a.l0_mfma = tab ? copies + h.l0_mfma_offset : nullptr;
        a.stride = cstride;
        a.has_two = two;
        a.classes = reinterpret_cast<int32_t *>(res);
        a.words = reinterpret_cast<uint64_t *>(res);
        a.number_class = number_class;
        a.stream = r.stream;
        a.first = a.last = l;
        const hipError_t e = window ? act_window(net.id, l, a, r.d_sw_base + boff[(size_t)l - 1], window)
                             : cnv  ? run_cnv_multi(net.id, a)
                                    : run_lfc_multi(net.id, a);
        if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
      }
      return 0;
    };
    // -- the fault-free pass, once: every layer's output and the results of all n images
    const uint8_t *const clean = static_cast<const uint8_t *>(r.d_blob);
    for (int i0 = 0; i0 < n; i0 += kMaxChunk) {
      const int m = std::min(kMaxChunk, n - i0);
      if (begin()) return -1;
      segs.assign(1, MultiSeg{0, i0, 0, m});
      if (plan()) return -1;
      for (int l = 0; l < S; l++) {
        if (stage(l, clean, stride, base_two > 0, base_res)) return -1;
        if (l + 1 < S)
          HIP_OK(hipMemcpyAsync(r.d_sw_base + boff[(size_t)l] + (size_t)i0 * ob[(size_t)l], bufs[obuf[(size_t)l]], (size_t)m * ob[(size_t)l],
                                hipMemcpyDeviceToDevice, r.stream));
      }
      if (finish()) return -1;
    }
    if (!cnv) {  // (LFC: the classes are decoded on the host, like the campaign path)
      words.resize((size_t)n);
      HIP_OK(hipMemcpy(words.data(), base_res, (size_t)n * 8, hipMemcpyDeviceToHost));
      for (int i = 0; i < n; i++) base_cls[(size_t)i] = lfc_class_batched(words[(size_t)i], number_class);
    }
    // -- the runs' blob copies (parameter faults)
    if (begin()) return -1;
    if (!unpatched) {
      HIP_OK(hipMemcpyAsync(r.d_copies, r.d_blob, blob.size(), hipMemcpyDeviceToDevice, r.stream));
      for (size_t have = 1; have < (size_t)max_runs; have *= 2) {  // replicate by doubling
        const size_t c = std::min(have, (size_t)max_runs - have);
        HIP_OK(hipMemcpyAsync(r.d_copies + have * stride, r.d_copies, c * stride, hipMemcpyDeviceToDevice, r.stream));
      }
    }
    // -- run groups: g faults of one layer L, one per copy; window by window of the images
    for (int L = 0; L < S; L++) {
      const std::vector<int> &idx = by_layer[(size_t)L];
      for (size_t c0 = 0; c0 < idx.size(); c0 += (size_t)G[(size_t)L]) {
        const int g = (int)std::min<size_t>((size_t)G[(size_t)L], idx.size() - c0), s0 = start_of(L);
        // host: each fault's patch (the rebuilt row; layer 0: and the MFMA table) and the original bytes it replaces
        std::vector<uint8_t> staging;
        std::vector<PatchSpan> patch, undo;
        bool two = base_two > 0;
        hipError_t e = hipSuccess;
        const PatchSpan *d_spans = nullptr;
        const ActPatch *d_sites = nullptr;
        const ActWinSite *d_wsites = nullptr;
        const bool wnd = windowed(L);
        if (wnd) {  // activation sites of CNV layers 0..2: each run's site as the window kernels change it
          std::vector<ActWinSite> ws((size_t)g);
          for (int q = 0; q < g; q++) {
            const ActSite &st = (*sites)[(size_t)idx[c0 + (size_t)q]];
            ws[(size_t)q] = ActWinSite{st.y, st.x, st.channel / 64, st.channel % 64, st.shift, {0, 0, 0}};
          }
          upload.assign(ws.size() * sizeof(ActWinSite), 0);
          std::memcpy(upload.data(), ws.data(), upload.size());
          if (r.d_sw_stage.grow(upload.size()) || begin()) return -1;
          HIP_OK(hipMemcpyAsync(r.d_sw_stage, upload.data(), upload.size(), hipMemcpyHostToDevice, r.stream));
          d_wsites = reinterpret_cast<const ActWinSite *>(r.d_sw_stage.get());
        } else if (inp) {  // input sites: each run's bit as k_input_seed flips it (the image's 16-byte lane, the bit inside it)
          std::vector<ActPatch> ap((size_t)g);
          for (int q = 0; q < g; q++) {
            const InputSite &st = (*inputs)[(size_t)idx[c0 + (size_t)q]];
            ap[(size_t)q] = ActPatch{(uint32_t)st.byte / 16, ((uint32_t)st.byte % 16) * 8 + (uint32_t)st.bit, 0, 0};
          }
          upload.assign(ap.size() * sizeof(ActPatch), 0);
          std::memcpy(upload.data(), ap.data(), upload.size());
          if (r.d_sw_stage.grow(upload.size()) || begin()) return -1;
          HIP_OK(hipMemcpyAsync(r.d_sw_stage, upload.data(), upload.size(), hipMemcpyHostToDevice, r.stream));
          d_sites = reinterpret_cast<const ActPatch *>(r.d_sw_stage.get());
        } else if (act) {  // activation sites: each run's site as k_act_seed patches it
          ActShape sh{};
          act_shape(net, L, &sh);
          const bool two_bit = sh.levels == 3;
          std::vector<ActPatch> ap((size_t)g);
          for (int q = 0; q < g; q++) {
            const ActSite &st = (*sites)[(size_t)idx[c0 + (size_t)q]];
            const uint32_t pix = (uint32_t)(st.y * sh.w + st.x), c = (uint32_t)st.channel;
            if (two_bit) {  // [pixel][C/64][sign, non-zero] u64: one 16-byte unit per 64 channels
              ap[(size_t)q] = ActPatch{pix * (uint32_t)(sh.c / 64) + c / 64, c % 64, (uint32_t)st.shift, 0};
            } else {  // [pixel][C/32] dwords: four per unit
              const uint32_t d = pix * (uint32_t)(sh.c / 32) + c / 32;
              ap[(size_t)q] = ActPatch{d / 4, (d % 4) * 32 + c % 32, (uint32_t)st.shift, 0};
            }
          }
          upload.assign(ap.size() * sizeof(ActPatch), 0);
          std::memcpy(upload.data(), ap.data(), upload.size());
          if (r.d_sw_stage.grow(upload.size()) || begin()) return -1;
          HIP_OK(hipMemcpyAsync(r.d_sw_stage, upload.data(), upload.size(), hipMemcpyHostToDevice, r.stream));
          d_sites = reinterpret_cast<const ActPatch *>(r.d_sw_stage.get());
        } else {  // parameter faults: the patches of the group's copies
          auto add_span = [&](int q, size_t off, size_t bytes) {
            patch.push_back(PatchSpan{(uint64_t)q * stride + off, (uint32_t)staging.size(), (uint32_t)bytes});
            staging.insert(staging.end(), blob.begin() + off, blob.begin() + off + bytes);
            undo.push_back(PatchSpan{(uint64_t)q * stride + off, (uint32_t)staging.size(), (uint32_t)bytes});
            staging.insert(staging.end(), r.blob.begin() + off, r.blob.begin() + off + bytes);
          };
          for (int q = 0; q < g; q++) {
            const Fault &flt = (*faults)[(size_t)idx[c0 + (size_t)q]];
            uint64_t *w = fault_word(net, raw, flt);
            const uint64_t old = *w;
            const int row = apply_fault(net, raw, flt);
            const int before = two_flag(L, row);
            size_t off = 0, bytes = 0;
            repack_row(net, raw, L, row, blob, &off, &bytes);
            if (base_two + two_flag(L, row) - before > 0) two = true;
            if (L == 0 && h.l0_mfma_offset) {  // repack_row's span runs from the row to the table's end: the two parts
              const size_t rbytes = (size_t)h.layer[0].row_dwords * 4;
              add_span(q, h.layer[0].offset + (size_t)row * rbytes, rbytes);
              if (tab) add_span(q, h.l0_mfma_offset, kL0MfmaBytes);
            } else {
              add_span(q, off, bytes);
            }
            *w = old;
            repack_row(net, raw, L, row, blob, &off, &bytes);
          }
          const size_t spans_off = (staging.size() + 255) & ~(size_t)255;
          upload.assign(spans_off + (patch.size() + undo.size()) * sizeof(PatchSpan), 0);
          std::memcpy(upload.data(), staging.data(), staging.size());
          std::memcpy(upload.data() + spans_off, patch.data(), patch.size() * sizeof(PatchSpan));
          std::memcpy(upload.data() + spans_off + patch.size() * sizeof(PatchSpan), undo.data(), undo.size() * sizeof(PatchSpan));
          if (r.d_sw_stage.grow(upload.size()) || begin()) return -1;
          HIP_OK(hipMemcpyAsync(r.d_sw_stage, upload.data(), upload.size(), hipMemcpyHostToDevice, r.stream));
          d_spans = reinterpret_cast<const PatchSpan *>(r.d_sw_stage + spans_off);
          e = scatter_patches(r.d_sw_stage, d_spans, (int)patch.size(), r.d_copies, r.stream);
          if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
        }
        if (act && trace().on)
          std::fprintf(stderr, "bnn-mi355x trace act_fault_sweep: layer %d sites %zu..%zu of %zu, window %d of %d images\n", L, c0, c0 + g - 1,
                       idx.size(), std::min(win[(size_t)L], n), n);
        if (act && trace().on)
          std::fprintf(stderr, "bnn-mi355x trace act_fault_sweep window: layer %d, %lld pairs windowed, %d pixels per pair\n", L,
                       wnd ? (long long)g * n : 0LL, wnd ? act_window_pixels(s0) : 0);
        const int wl = win[(size_t)L];
        for (int i0 = 0; i0 < n; i0 += wl) {
          const int m = std::min(wl, n - i0);  // (g > 1: m = n)
          if (begin()) return -1;
          // the runs start from the fault-free output of layer s0-1 (slot q * m + j) and the fault-free results; activation
          // sites: with the site changed (k_act_seed, below), or -- windowed -- from the fault-free output of layer s0 itself
          if (wnd) {
            const size_t bb = ob[(size_t)s0];
            e = sweep_broadcast(r.d_sw_base + boff[(size_t)s0] + (size_t)i0 * bb, bb, m, g, bufs[obuf[(size_t)s0]], (size_t)m * bb, r.stream);
            if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
          }
          if (!act && L > 0) {
            const size_t bb = ob[(size_t)L - 1];
            e = sweep_broadcast(r.d_sw_base + boff[(size_t)L - 1] + (size_t)i0 * bb, bb, m, g, bufs[obuf[(size_t)L - 1]], (size_t)m * bb, r.stream);
            if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
          }
          e = sweep_broadcast(base_res + (size_t)i0 * rb, rb, m, g, r.d_sw_res + (size_t)i0 * rb, (size_t)n * rb, r.stream);
          if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
          segs.clear();
          for (int q = 0; q < g; q++) segs.push_back(MultiSeg{q, i0, q * m, m});
          for (int l = s0; l < S; l++) {
            if (plan()) return -1;
            const ActWinSite *const window = (wnd && l == s0) ? d_wsites : nullptr;  // (in place of k_act_seed + the whole stage)
            if (act && l == s0 && !window) {
              e = act_seed(r.d_sw_base + boff[(size_t)L], (int)ob[(size_t)L], net.L[L].out_planes == 2, d_segs, (int)segs.size(), m, d_sites,
                           bufs[obuf[(size_t)L]], r.stream);
              if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
            }
            const bool from_staged = inp && l == 0;
            if (from_staged) {  // the group's faulted images, and layer 0's records: the same segments, their image the staged slot
              e = input_seed(r.d_all, (int)isz, d_segs, (int)segs.size(), m, d_sites, r.d_in_stage, r.stream);
              if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
              seed_segs = segs;
              for (MultiSeg &sg : seed_segs) sg.image = sg.slot;
              HIP_OK(hipMemcpyAsync(d_seed_segs, seed_segs.data(), seed_segs.size() * sizeof(MultiSeg), hipMemcpyHostToDevice, r.stream));
            }
            if (unpatched ? stage(l, clean, 0, two, r.d_sw_res, window, from_staged ? r.d_in_stage : nullptr, d_seed_segs)
                          : stage(l, r.d_copies, stride, two, r.d_sw_res))
              return -1;
            if (l == s0) pairs[(size_t)l] += (long)g * m;
            if (l + 1 == S) break;
            // prune: only the (run, image) pairs whose output differs from the fault-free one go on (and the gaps between them below `bridge`)
            HIP_OK(hipMemsetAsync(r.d_sw_alive, 0, (size_t)g * m, r.stream));
            if (profile) HIP_OK(hipMemsetAsync(r.d_sw_prof, 0, (size_t)g * 16, r.stream));
            for (const Batch &b : batches) {
              e = profile ? sweep_profile(bufs[obuf[(size_t)l]], r.d_sw_base + boff[(size_t)l], (int)ob[(size_t)l], net.L[l].out_planes == 2,
                                          d_segs + b.seg0, b.nsegs, b.max_len, r.d_sw_alive,
                                          reinterpret_cast<unsigned long long *>(r.d_sw_prof.get()), r.stream)
                          : sweep_mark(bufs[obuf[(size_t)l]], r.d_sw_base + boff[(size_t)l], (int)ob[(size_t)l], d_segs + b.seg0, b.nsegs, b.max_len,
                                       r.d_sw_alive, r.stream);
              if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
            }
            alive.resize((size_t)g * m);
            HIP_OK(hipMemcpyAsync(alive.data(), r.d_sw_alive, alive.size(), hipMemcpyDeviceToHost, r.stream));
            if (profile) {
              prof.resize((size_t)g * 2);
              HIP_OK(hipMemcpyAsync(prof.data(), r.d_sw_prof, (size_t)g * 16, hipMemcpyDeviceToHost, r.stream));
            }
            if (finish()) return -1;
            for (int q = 0; profile && q < g; q++) {  // (g = 1: a fault's images come window by window)
              const size_t at = (size_t)idx[c0 + (size_t)q] * (size_t)(S - 1) + (size_t)l;
              prof_alive[at] += (long)prof[2 * (size_t)q];
              prof_flipped[at] += (long)prof[2 * (size_t)q + 1];
            }
            // the survivors as segments, cut from the records that just ran; a gap shorter than the next stage's smallest
            // grid per record (8 blocks of work items, map_block) is run through rather than cut: a pair that ran this
            // stage with the fault-free output gives the fault-free outputs again, and a record costs that grid however
            // short it is.  (Never across records: a pair dropped earlier holds stale activations.)
            const int bridge = std::max(1, 8 * 256 / ipi[(size_t)l + 1]);
            ran.swap(segs);
            segs.clear();
            for (const MultiSeg &sg : ran) {
              const uint8_t *al = alive.data() + sg.slot;
              int b = -1, e2 = -1;  // the open segment [b, e2) of this record
              for (int j = 0; j < sg.len;) {
                uint64_t z;
                if (j + 8 <= sg.len && (std::memcpy(&z, al + j, 8), z == 0)) { j += 8; continue; }
                if (!al[j]) { j++; continue; }
                if (b >= 0 && j - e2 >= bridge) {
                  segs.push_back(MultiSeg{sg.run, sg.image + b, sg.slot + b, e2 - b});
                  b = -1;
                }
                if (b < 0) b = j;
                const int a0 = j;
                while (j < sg.len && al[j]) j++;
                pairs[(size_t)l + 1] += j - a0;
                e2 = j;
              }
              if (b >= 0) segs.push_back(MultiSeg{sg.run, sg.image + b, sg.slot + b, e2 - b});
            }
            if (segs.empty()) break;
            if (begin()) return -1;
          }
          // classes against the fault-free ones (pairs pruned at any layer kept the fault-free result)
          if (begin()) return -1;
          if (cnv) {
            const int32_t *cls = reinterpret_cast<const int32_t *>(r.d_sw_res.get()) + i0, *bcls = reinterpret_cast<const int32_t *>(base_res) + i0;
            e = sweep_count(cls, bcls, n, m, g, d_counts, r.stream);
            if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
            counts.resize((size_t)g);
            HIP_OK(hipMemcpyAsync(counts.data(), d_counts, (size_t)g * 4, hipMemcpyDeviceToHost, r.stream));
            if (finish()) return -1;
            offs.assign((size_t)g, 0);
            long long tot = 0;
            for (int q = 0; q < g; q++) {
              offs[(size_t)q] = tot;
              tot += counts[(size_t)q];
            }
            pv.resize((size_t)tot * 2);
            if (tot > 0 && cap_diffs > 0) {
              if (begin()) return -1;
              HIP_OK(hipMemcpyAsync(d_offsets, offs.data(), (size_t)g * 8, hipMemcpyHostToDevice, r.stream));
              e = sweep_emit(cls, bcls, n, m, g, d_counts, d_offsets, reinterpret_cast<int *>(r.d_sw_diffs.get()), r.stream);
              if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
              HIP_OK(hipMemcpyAsync(pv.data(), r.d_sw_diffs, (size_t)tot * 8, hipMemcpyDeviceToHost, r.stream));
              if (finish()) return -1;
              for (size_t k = 0; k < (size_t)tot; k++) pv[2 * k] += i0;
            }
            for (int q = 0; q < g; q++) {
              const int fi = idx[c0 + (size_t)q];
              changed[fi] += counts[(size_t)q];
              total_changed += counts[(size_t)q];
              keep(fi, pv.data() + 2 * offs[(size_t)q], counts[(size_t)q]);
            }
          } else {  // (LFC: the raw words back, decoded on the host)
            const size_t span = (size_t)(g - 1) * n + m;
            words.resize(span);
            HIP_OK(hipMemcpyAsync(words.data(), r.d_sw_res + (size_t)i0 * 8, span * 8, hipMemcpyDeviceToHost, r.stream));
            if (finish()) return -1;
            for (int q = 0; q < g; q++) {
              const int fi = idx[c0 + (size_t)q];
              pv.clear();
              for (int j = 0; j < m; j++) {
                const int c = lfc_class_batched(words[(size_t)q * n + j], number_class);
                if (c != base_cls[(size_t)i0 + j]) { pv.push_back(i0 + j); pv.push_back(c); }
              }
              const long cnt = (long)pv.size() / 2;
              changed[fi] += (int)cnt;
              total_changed += cnt;
              keep(fi, pv.data(), cnt);
            }
          }
        }
        // the copies back to the loaded parameters
        if (unpatched) continue;
        if (begin()) return -1;
        e = scatter_patches(r.d_sw_stage, d_spans + patch.size(), (int)undo.size(), r.d_copies, r.stream);
        if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
      }
    }
    if (finish()) return -1;
    drain.ok();
    return 0;
  };
  if (run() < 0) return -1;
  if (profile) {
    r.prof_alive = std::move(prof_alive);
    r.prof_flipped = std::move(prof_flipped);
    r.prof_rows = n_faults;
    r.prof_cols = S - 1;
  }
  long k = 0;
  for (auto &e : kept)
    for (size_t i = 0; i + 1 < e.second.size() && k < cap_diffs; i += 2, k++) {
      diffs[3 * k] = e.first;
      diffs[3 * k + 1] = e.second[i];
      diffs[3 * k + 2] = e.second[i + 1];
    }
  stage_pairs = std::move(pairs);
  if (image_number) *image_number = n;
  if (usecPerImage) *usecPerImage = (n > 0 && n_faults > 0) ? (float)(device_us / ((double)n_faults * n)) : 0.f;
  return total_changed;
}

long bnn_mi355x_fault_sweep(const char *path, int number_class, const int *records, int n_faults, int *changed, int *diffs,
                            long cap_diffs, int *image_number, float *usecPerImage) {
  Runtime &r = rt();
  r.sweep_pairs.clear();
  sweep_profile_begin(r);
  if (n_faults < 0 || (n_faults > 0 && (!records || !changed)) || cap_diffs < 0 || (cap_diffs > 0 && !diffs))
    return fail("fault_sweep: bad arguments (records / changed missing, or cap_diffs without diffs)");
#ifdef BNN_VARIANT
  return fail("fault injection is not modelled for " BNN_VARIANT " (replicated / interleaved parameter memories); use the base network");
#endif
  if (!ready()) return -1;
  if (r.raw.empty()) return fail("fault injection needs the parameter files (load_parameters), not an imported blob");
  if (r.l1_mfma || r.l1_literal)
    return fail("fault injection is not wired to the BNN_MI355X_L1 comparison forms (the matrix-pipe table is not patched)");
  const NetSpec &net = r.spec;
  std::vector<Fault> faults((size_t)n_faults);
  for (int i = 0; i < n_faults; i++) {
    faults[(size_t)i] = fault_record(records + (size_t)i * 8);
    faults[(size_t)i].image = 0;  // (whatever the record's first int holds)
    const std::string e = check_fault(net, faults[(size_t)i]);
    if (!e.empty()) return fail("fault_sweep: record " + std::to_string(i) + ": " + e);
  }
  return single_fault_sweep(path, number_class, &faults, nullptr, nullptr, changed, diffs, cap_diffs, image_number, usecPerImage, r.sweep_pairs);
}

int bnn_mi355x_last_sweep_stages(long *pairs_per_stage, int cap) {
  const std::vector<long> &p = rt().sweep_pairs;
  for (int i = 0; pairs_per_stage && i < cap && i < (int)p.size(); i++) pairs_per_stage[i] = p[(size_t)i];
  return (int)p.size();
}

int bnn_mi355x_sweep_profile(int enable) {
  Runtime &r = rt();
  const int before = r.sweep_profile ? 1 : 0;
  r.sweep_profile = enable != 0;
  return before;
}

long bnn_mi355x_last_sweep_profile(long first, long *alive, long *flipped, long cap_rows, int *columns) {
  const Runtime &r = rt();
  if (first < 0) return fail("last_sweep_profile: negative first");
  if (columns) *columns = r.spec.nlayers - 1;
  const size_t cols = (size_t)r.prof_cols;
  for (long i = first; i < r.prof_rows && i - first < cap_rows; i++) {
    if (alive) std::memcpy(alive + (size_t)(i - first) * cols, r.prof_alive.data() + (size_t)i * cols, cols * sizeof(long));
    if (flipped) std::memcpy(flipped + (size_t)(i - first) * cols, r.prof_flipped.data() + (size_t)i * cols, cols * sizeof(long));
  }
  return r.prof_rows;
}

long bnn_mi355x_enumerate_act_faults(int layer, long first, int *records, int cap_records) {
  const NetSpec &net = rt().spec;
  const long total = enumerate_act_faults(net, layer, 0, nullptr, 0);
  if (total < 0 || first < 0)
    return fail("enumerate_act_faults: bad layer (0 ... " + std::to_string(net.nlayers - 2) + ": the last layer has no activations) or first");
  if (records && cap_records > 0 && first < total) {
    std::vector<ActSite> v((size_t)std::min<long>(cap_records, total - first));
    enumerate_act_faults(net, layer, first, v.data(), (long)v.size());
    for (size_t i = 0; i < v.size(); i++) {
      const int w[5] = {v[i].layer, v[i].y, v[i].x, v[i].channel, v[i].shift};
      std::memcpy(records + i * 5, w, sizeof w);
    }
  }
  return total;
}

long bnn_mi355x_act_fault_sweep(const char *path, int number_class, const int *records, int n_faults, int *changed, int *diffs,
                                long cap_diffs, int *image_number, float *usecPerImage) {
  Runtime &r = rt();
  r.act_sweep_pairs.clear();
  sweep_profile_begin(r);
  if (n_faults < 0 || (n_faults > 0 && (!records || !changed)) || cap_diffs < 0 || (cap_diffs > 0 && !diffs))
    return fail("act_fault_sweep: bad arguments (records / changed missing, or cap_diffs without diffs)");
#ifdef BNN_VARIANT
  return fail("fault injection is not modelled for " BNN_VARIANT " (replicated / interleaved parameter memories); use the base network");
#endif
  const NetSpec &net = r.spec;
  std::vector<ActSite> sites((size_t)n_faults);
  for (int i = 0; i < n_faults; i++) {  // (host only: before anything runs on the device)
    const int *v = records + (size_t)i * 5;
    sites[(size_t)i] = ActSite{v[0], v[1], v[2], v[3], v[4]};
    const std::string e = check_act_fault(net, sites[(size_t)i]);
    if (!e.empty())
      return fail("act_fault_sweep: record " + std::to_string(i) + " {" + std::to_string(v[0]) + ", " + std::to_string(v[1]) + ", " +
                  std::to_string(v[2]) + ", " + std::to_string(v[3]) + ", " + std::to_string(v[4]) + "}: " + e);
  }
  if (!ready()) return -1;
  if (r.l1_mfma || r.l1_literal)
    return fail("fault injection is not wired to the BNN_MI355X_L1 comparison forms (the sweeps run the standard multi-run stages)");
  return single_fault_sweep(path, number_class, nullptr, &sites, nullptr, changed, diffs, cap_diffs, image_number, usecPerImage, r.act_sweep_pairs);
}

int bnn_mi355x_last_act_sweep_stages(long *pairs_per_stage, int cap) {
  const std::vector<long> &p = rt().act_sweep_pairs;
  for (int i = 0; pairs_per_stage && i < cap && i < (int)p.size(); i++) pairs_per_stage[i] = p[(size_t)i];
  return (int)p.size();
}

// Random activation upsets, many runs in one call.  The work items are (run, image) pairs in run-major order, cut into
// groups of at most one activation workspace; every group runs every layer's MULTI stage on the loaded blob (copy stride
// 0, the integer-pipe kernels of the fault paths) with k_act_noise between two stages where the layer's rate is not 0.
// The draw keys on the image's index in the file, so the grouping never shows in the results.
int *bnn_mi355x_act_noise_campaigns(const char *path, int number_class, int num_runs, unsigned long long seed,
                                    const unsigned int *rate_q32, int n_rates, int *image_number, float *usecPerImage) {
  Runtime &r = rt();
  const NetSpec &net = r.spec;
  r.noise_counts.clear();
  r.noise_seeds.clear();
  const int S = net.nlayers;
  if (!path || !rate_q32 || n_rates != S - 1) {
    fail("act_noise_campaigns: bad arguments (path / rate_q32 missing, or n_rates is not " + std::to_string(S - 1) + ": one rate per layer but the last)");
    return nullptr;
  }
  if (num_runs < 1 || num_runs > kMaxRuns) {
    fail("act_noise_campaigns: num_runs must be 1 ... " + std::to_string(kMaxRuns));
    return nullptr;
  }
  const int R = num_runs;
  if (seed != 0 && 0ull - (uint64_t)seed < (uint64_t)R) {
    fail("act_noise_campaigns: seed + run wraps to 0 for a run (0 seeds from std::random_device)");
    return nullptr;
  }
#ifdef BNN_VARIANT
  fail("fault injection is not modelled for " BNN_VARIANT " (replicated / interleaved parameter memories); use the base network");
  return nullptr;
#endif
  if (!ready()) return nullptr;
  if (r.l1_mfma || r.l1_literal) {
    fail("fault injection is not wired to the BNN_MI355X_L1 comparison forms (the campaigns run the standard multi-run stages)");
    return nullptr;
  }
  ImageFile f;
  if (open_image_file(path, f)) return nullptr;
  const int n = (int)f.n;
  const size_t total = (size_t)R * n;
  const bool cnv = net.is_cnv;
  std::vector<unsigned long long> seeds((size_t)R);
  {
    std::random_device rd;
    for (int q = 0; q < R; q++) {
      unsigned long long k = seed ? seed + (unsigned long long)q : 0;  // (seed 0: every run from std::random_device, never 0)
      while (k == 0) k = ((unsigned long long)rd() << 32) | rd();
      seeds[(size_t)q] = k;
    }
  }
  int *result = new (std::nothrow) int[total + 1];
  if (!result) { fail("out of memory"); return nullptr; }
  std::vector<unsigned long long> counts((size_t)R * (S - 1), 0);
  double device_us = 0.0;
  auto run = [&]() -> int {
    if (n == 0) return 0;
    size_t cap = std::min<size_t>(kMaxChunk, total);  // pairs per group: the activation workspace
    if (const char *e = std::getenv("BNN_MI355X_NOISE_GROUP")) {  // tests: many small groups
      const long long v = std::atoll(e);
      if (v > 0) cap = std::min<size_t>(cap, (size_t)v);
    }
    std::vector<size_t> ob((size_t)S, 0);
    std::vector<int> obuf((size_t)S, 0);
    for (int l = 0; l + 1 < S; l++) ob[(size_t)l] = stage_output_bytes(cnv, net.abits, cnv ? l : l + 1, &obuf[(size_t)l]);
    // the records of every group: a run's images, cut at the group's end
    struct Group { size_t seg0; int nsegs, max_len, total; };
    std::vector<MultiSeg> segs;
    std::vector<Group> groups;
    for (size_t p0 = 0; p0 < total; p0 += cap) {
      const size_t p1 = std::min(total, p0 + cap);
      Group g{segs.size(), 0, 0, 0};
      for (size_t p = p0; p < p1;) {
        const int q = (int)(p / (size_t)n), i = (int)(p % (size_t)n), m = (int)std::min<size_t>((size_t)(n - i), p1 - p);
        segs.push_back(MultiSeg{q, i, g.total, m});
        g.nsegs++;
        g.total += m;
        g.max_len = std::max(g.max_len, m);
        p += (size_t)m;
      }
      groups.push_back(g);
    }
    PackedHeader h;
    std::memcpy(&h, r.blob.data(), sizeof(h));
    const bool tab = h.l0_mfma_offset && r.l0_mfma;
    const size_t counts_off = ((size_t)R * 8 + 255) & ~(size_t)255;
    if (load_file_resident(f, n) || reserve((int)cap)) return -1;
    if (r.d_sw_segs.grow(segs.size() * sizeof(MultiSeg)) || r.d_noise.grow(counts_off + counts.size() * 8) ||
        r.d_camp_res.grow(total * (cnv ? sizeof(int32_t) : sizeof(uint64_t))))
      return -1;
    const unsigned long long *const d_seeds = reinterpret_cast<const unsigned long long *>(r.d_noise.get());
    unsigned long long *const d_counts = reinterpret_cast<unsigned long long *>(r.d_noise + counts_off);
    const MultiSeg *const d_segs = reinterpret_cast<const MultiSeg *>(r.d_sw_segs.get());
    uint8_t *const bufs[2] = {static_cast<uint8_t *>(r.buf0), static_cast<uint8_t *>(r.buf1)};
    const uint8_t *const clean = static_cast<const uint8_t *>(r.d_blob);
    std::vector<uint64_t> w;  // (LFC: raw words, decoded on the host)
    if (!cnv) w.resize(total);
    DrainOnFailure drain;  // (declared after the host buffers the queued copies read or write)
    if (settle_handover(r.stream)) return -1;
    while (r.time_events.size() < 2) {
      hipEvent_t e;
      HIP_OK(hipEventCreateWithFlags(&e, kTimeEventFlags));
      r.time_events.push_back(e);
    }
    // -- all of it on one stream, one wait at the end
    HIP_OK(hipEventRecord(r.time_events[0], r.stream));
    HIP_OK(hipMemcpyAsync(r.d_noise, seeds.data(), (size_t)R * 8, hipMemcpyHostToDevice, r.stream));
    HIP_OK(hipMemsetAsync(d_counts, 0, counts.size() * 8, r.stream));
    HIP_OK(hipMemcpyAsync(r.d_sw_segs, segs.data(), segs.size() * sizeof(MultiSeg), hipMemcpyHostToDevice, r.stream));
    for (const Group &g : groups) {
      for (int l = 0; l < S; l++) {
        MultiLaunch a{};
        a.images = r.d_all;
        a.segs = d_segs + g.seg0;
        a.nsegs = g.nsegs; a.max_len = g.max_len; a.total = g.total; a.n = n;
        a.buf0 = r.buf0; a.buf1 = r.buf1;
        for (int k = 0; k < S; k++) a.rows[k] = reinterpret_cast<const uint32_t *>(clean + h.layer[k].offset);
        a.l0_mfma = tab ? clean + h.l0_mfma_offset : nullptr;
        a.stride = 0;  // every run reads the one loaded blob
        a.has_two = r.two_rows > 0;
        a.classes = reinterpret_cast<int32_t *>(r.d_camp_res.get());
        a.words = reinterpret_cast<uint64_t *>(r.d_camp_res.get());
        a.number_class = number_class;
        a.stream = r.stream;
        a.first = a.last = l;
        hipError_t e = cnv ? run_cnv_multi(net.id, a) : run_lfc_multi(net.id, a);
        if (e == hipSuccess && l + 1 < S)
          e = act_noise(bufs[obuf[(size_t)l]], (int)ob[(size_t)l], net.L[l].out_planes == 2, a.segs, g.nsegs, g.max_len, d_seeds, l,
                        rate_q32[l], d_counts, S - 1, r.stream);
        if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
      }
    }
    HIP_OK(hipEventRecord(r.time_events[1], r.stream));
    HIP_OK(hipMemcpyAsync(counts.data(), d_counts, counts.size() * 8, hipMemcpyDeviceToHost, r.stream));
    if (cnv) HIP_OK(hipMemcpyAsync(result, r.d_camp_res, total * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
    else HIP_OK(hipMemcpyAsync(w.data(), r.d_camp_res, total * sizeof(uint64_t), hipMemcpyDeviceToHost, r.stream));
    HIP_OK(hipStreamSynchronize(r.stream));
    for (size_t i = 0; !cnv && i < total; i++) result[i] = lfc_class_batched(w[i], number_class);
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, r.time_events[0], r.time_events[1]));
    drain.ok();
    device_us = ms * 1000.0;
    return 0;
  };
  if (run() < 0) {
    delete[] result;
    return nullptr;
  }
  r.noise_counts.assign(counts.begin(), counts.end());
  r.noise_seeds = std::move(seeds);
  if (image_number) *image_number = n;
  if (usecPerImage) *usecPerImage = total ? (float)(device_us / (double)total) : 0.f;
  return result;
}

int bnn_mi355x_last_act_noise_counts(long *upsets, int cap) {
  const std::vector<long> &c = rt().noise_counts;
  for (int i = 0; upsets && i < cap && i < (int)c.size(); i++) upsets[i] = c[(size_t)i];
  return (int)c.size();
}

int bnn_mi355x_last_act_noise_seeds(unsigned long long *seeds, int cap) {
  const std::vector<unsigned long long> &k = rt().noise_seeds;
  for (int i = 0; seeds && i < cap && i < (int)k.size(); i++) seeds[i] = k[(size_t)i];
  return (int)k.size();
}

long bnn_mi355x_act_noise_mask(unsigned long long run_seed, int image, int layer, unsigned int rate_q32, long first, int *records,
                               int cap_records) {
  const NetSpec &net = rt().spec;
  const long total = act_noise_mask(net, run_seed, image, layer, rate_q32, 0, nullptr, 0);
  if (total < 0 || first < 0 || image < 0)
    return fail("act_noise_mask: bad layer (0 ... " + std::to_string(net.nlayers - 2) + ": the last layer has no activations), image or first");
  if (records && cap_records > 0 && first < total) {
    std::vector<ActSite> v((size_t)std::min<long>(cap_records, total - first));
    act_noise_mask(net, run_seed, image, layer, rate_q32, first, v.data(), (long)v.size());
    for (size_t i = 0; i < v.size(); i++) {
      const int w[5] = {v[i].layer, v[i].y, v[i].x, v[i].channel, v[i].shift};
      std::memcpy(records + i * 5, w, sizeof w);
    }
  }
  return total;
}

long bnn_mi355x_enumerate_input_faults(long first, int *records, int cap_records) {
  const NetSpec &net = rt().spec;
  const long total = input_sites(net);
  if (first < 0) return fail("enumerate_input_faults: first must not be negative");
  if (records && cap_records > 0 && first < total) {
    std::vector<InputSite> v((size_t)std::min<long>(cap_records, total - first));
    enumerate_input_faults(net, first, v.data(), (long)v.size());
    for (size_t i = 0; i < v.size(); i++) {
      records[2 * i] = v[i].byte;
      records[2 * i + 1] = v[i].bit;
    }
  }
  return total;
}

long bnn_mi355x_input_fault_sweep(const char *path, int number_class, const int *records, int n_faults, int *changed, int *diffs,
                                  long cap_diffs, int *image_number, float *usecPerImage) {
  Runtime &r = rt();
  r.input_sweep_pairs.clear();
  sweep_profile_begin(r);
  if (!path || n_faults < 0 || (n_faults > 0 && (!records || !changed)) || cap_diffs < 0 || (cap_diffs > 0 && !diffs) || number_class < 1 ||
      number_class > 64)
    return fail("input_fault_sweep: bad arguments (path / records / changed missing, cap_diffs without diffs, or number_class outside 1 ... 64)");
#ifdef BNN_VARIANT
  return fail("fault injection is not modelled for " BNN_VARIANT " (replicated / interleaved parameter memories); use the base network");
#endif
  const NetSpec &net = r.spec;
  std::vector<InputSite> sites((size_t)n_faults);
  for (int i = 0; i < n_faults; i++) {  // (host only: before anything runs on the device)
    const int *v = records + (size_t)i * 2;
    sites[(size_t)i] = InputSite{v[0], v[1]};
    const std::string e = check_input_fault(net, sites[(size_t)i]);
    if (!e.empty()) return fail("input_fault_sweep: record " + std::to_string(i) + " {" + std::to_string(v[0]) + ", " + std::to_string(v[1]) + "}: " + e);
  }
  if (!ready()) return -1;
  if (r.l1_mfma || r.l1_literal)
    return fail("fault injection is not wired to the BNN_MI355X_L1 comparison forms (the sweeps run the standard multi-run stages)");
  return single_fault_sweep(path, number_class, nullptr, nullptr, &sites, changed, diffs, cap_diffs, image_number, usecPerImage,
                            r.input_sweep_pairs);
}

int bnn_mi355x_last_input_sweep_stages(long *pairs_per_stage, int cap) {
  const std::vector<long> &p = rt().input_sweep_pairs;
  for (int i = 0; pairs_per_stage && i < cap && i < (int)p.size(); i++) pairs_per_stage[i] = p[(size_t)i];
  return (int)p.size();
}

// Random input-buffer upsets, many runs in one call.  The work items are (run, image) pairs in run-major order, cut into
// groups of at most one staging buffer; k_input_noise writes a group's faulted images there (rate 0: plain copies, no
// upset launch) and the group is classified like any other batch of that many images in HBM -- the pass of
// bnn_mi355x_inference_device, matrix-core stages included, with the loaded parameters.  The draw keys on the image's
// index in the file, so the grouping never shows in the results.
int *bnn_mi355x_input_noise_campaigns(const char *path, int number_class, int num_runs, unsigned long long seed, unsigned int rate_q32,
                                      int *image_number, float *usecPerImage) {
  Runtime &r = rt();
  const NetSpec &net = r.spec;
  r.input_noise_counts.clear();
  r.input_noise_seeds.clear();
  if (!path || number_class < 1 || number_class > 64) {
    fail("input_noise_campaigns: bad arguments (path missing, or number_class outside 1 ... 64)");
    return nullptr;
  }
  if (num_runs < 1 || num_runs > kMaxRuns) {
    fail("input_noise_campaigns: num_runs must be 1 ... " + std::to_string(kMaxRuns));
    return nullptr;
  }
  const int R = num_runs;
  if (seed != 0 && 0ull - (uint64_t)seed < (uint64_t)R) {
    fail("input_noise_campaigns: seed + run wraps to 0 for a run (0 seeds from std::random_device)");
    return nullptr;
  }
#ifdef BNN_VARIANT
  fail("fault injection is not modelled for " BNN_VARIANT " (replicated / interleaved parameter memories); use the base network");
  return nullptr;
#endif
  if (!ready()) return nullptr;
  if (r.l1_mfma || r.l1_literal) {
    fail("fault injection is not wired to the BNN_MI355X_L1 comparison forms (a comparison figure's kernels, not a path to study)");
    return nullptr;
  }
  ImageFile f;
  if (open_image_file(path, f)) return nullptr;
  const int n = (int)f.n;
  const size_t total = (size_t)R * n;
  const bool cnv = net.is_cnv;
  std::vector<unsigned long long> seeds((size_t)R);
  {
    std::random_device rd;
    for (int q = 0; q < R; q++) {
      unsigned long long k = seed ? seed + (unsigned long long)q : 0;  // (seed 0: every run from std::random_device, never 0)
      while (k == 0) k = ((unsigned long long)rd() << 32) | rd();
      seeds[(size_t)q] = k;
    }
  }
  int *result = new (std::nothrow) int[total + 1];
  if (!result) { fail("out of memory"); return nullptr; }
  std::vector<unsigned long long> counts((size_t)R, 0);
  double device_us = 0.0;
  auto run = [&]() -> int {
    if (n == 0) return 0;
    size_t cap = std::min<size_t>(kInputStagePairs, total);  // pairs per group: the staging buffer
    if (const char *e = std::getenv("BNN_MI355X_NOISE_GROUP")) {  // tests: many small groups
      const long long v = std::atoll(e);
      if (v > 0) cap = std::min<size_t>(cap, (size_t)v);
    }
    const size_t isz = (size_t)net.image_bytes(), counts_off = ((size_t)R * 8 + 255) & ~(size_t)255;
    if (load_file_resident(f, n)) return -1;
    if (r.d_in_stage.grow(cap * isz + 256) || r.d_noise.grow(counts_off + counts.size() * 8) ||
        r.d_camp_res.grow(total * (cnv ? sizeof(int32_t) : sizeof(uint64_t))))
      return -1;
    const unsigned long long *const d_seeds = reinterpret_cast<const unsigned long long *>(r.d_noise.get());
    unsigned long long *const d_counts = reinterpret_cast<unsigned long long *>(r.d_noise + counts_off);
    std::vector<uint64_t> w;  // (LFC: raw words, decoded on the host)
    if (!cnv) w.resize(total);
    DrainOnFailure drain;  // (declared after the host buffers the queued copies read or write)
    if (settle_handover(r.stream)) return -1;
    while (r.time_events.size() < 2) {
      hipEvent_t e;
      HIP_OK(hipEventCreateWithFlags(&e, kTimeEventFlags));
      r.time_events.push_back(e);
    }
    // -- all of it on one stream, one wait at the end
    HIP_OK(hipEventRecord(r.time_events[0], r.stream));
    HIP_OK(hipMemcpyAsync(r.d_noise, seeds.data(), (size_t)R * 8, hipMemcpyHostToDevice, r.stream));
    HIP_OK(hipMemsetAsync(d_counts, 0, counts.size() * 8, r.stream));
    for (size_t p0 = 0; p0 < total; p0 += cap) {
      const int m = (int)std::min(cap, total - p0);
      if (rate_q32 != 0) {
        const hipError_t e = input_noise(r.d_all, (int)isz, p0, m, n, d_seeds, rate_q32, d_counts, r.d_in_stage, r.stream);
        if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
      } else {  // the same pairs through the same passes: each run's stretch of the group copied as it is
        for (size_t p = p0; p < p0 + (size_t)m;) {
          const size_t i = p % (size_t)n, len = std::min((size_t)n - i, p0 + (size_t)m - p);
          HIP_OK(hipMemcpyAsync(r.d_in_stage + (p - p0) * isz, r.d_all + i * isz, len * isz, hipMemcpyDeviceToDevice, r.stream));
          p += len;
        }
      }
      // (the device entry point itself, on the library's stream: whatever pass it takes for m images is the pass taken here)
      if (bnn_mi355x_inference_device(r.d_in_stage, m, number_class, cnv ? reinterpret_cast<int32_t *>(r.d_camp_res.get()) + p0 : nullptr, nullptr,
                                      cnv ? nullptr : reinterpret_cast<uint64_t *>(r.d_camp_res.get()) + p0, r.stream))
        return -1;
    }
    HIP_OK(hipEventRecord(r.time_events[1], r.stream));
    HIP_OK(hipMemcpyAsync(counts.data(), d_counts, counts.size() * 8, hipMemcpyDeviceToHost, r.stream));
    if (cnv) HIP_OK(hipMemcpyAsync(result, r.d_camp_res, total * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
    else HIP_OK(hipMemcpyAsync(w.data(), r.d_camp_res, total * sizeof(uint64_t), hipMemcpyDeviceToHost, r.stream));
    HIP_OK(hipStreamSynchronize(r.stream));
    for (size_t i = 0; !cnv && i < total; i++) result[i] = lfc_class_batched(w[i], number_class);
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, r.time_events[0], r.time_events[1]));
    drain.ok();
    device_us = ms * 1000.0;
    return 0;
  };
  if (run() < 0) {
    delete[] result;
    return nullptr;
  }
  r.input_noise_counts.assign(counts.begin(), counts.end());
  r.input_noise_seeds = std::move(seeds);
  if (image_number) *image_number = n;
  if (usecPerImage) *usecPerImage = total ? (float)(device_us / (double)total) : 0.f;
  return result;
}

int bnn_mi355x_last_input_noise_counts(long *upsets, int cap) {
  const std::vector<long> &c = rt().input_noise_counts;
  for (int i = 0; upsets && i < cap && i < (int)c.size(); i++) upsets[i] = c[(size_t)i];
  return (int)c.size();
}

int bnn_mi355x_last_input_noise_seeds(unsigned long long *seeds, int cap) {
  const std::vector<unsigned long long> &k = rt().input_noise_seeds;
  for (int i = 0; seeds && i < cap && i < (int)k.size(); i++) seeds[i] = k[(size_t)i];
  return (int)k.size();
}

long bnn_mi355x_input_noise_mask(unsigned long long run_seed, int image, unsigned int rate_q32, long first, int *records, int cap_records) {
  const NetSpec &net = rt().spec;
  if (first < 0 || image < 0) return fail("input_noise_mask: image and first must not be negative");
  const long total = input_noise_mask(net, run_seed, image, rate_q32, 0, nullptr, 0);
  if (records && cap_records > 0 && first < total) {
    std::vector<InputSite> v((size_t)std::min<long>(cap_records, total - first));
    input_noise_mask(net, run_seed, image, rate_q32, first, v.data(), (long)v.size());
    for (size_t i = 0; i < v.size(); i++) {
      records[2 * i] = v[i].byte;
      records[2 * i + 1] = v[i].bit;
    }
  }
  return total;
}

// ---- memory upset-rate campaigns (the model: mem_faults.h) ---------------------------------------------------------------

// the argument checks of both entry points, then what every parameter-fault entry point refuses; nothing touches a device
// before they have passed (ready() is the first thing that may)
// hz: the memory organisation (mem_org.h) -- the plain entry points pass scheme 0 with burst 1, which every network has
// code: the SEC-DED axis of bnn_mi355x_ecc_exposure_campaigns (ecc.h); 0 everywhere else
// base_only: a variant's library refuses the entry point (the plain ones: the organisation is the variant's there, not
// an argument; where the scheme is an argument the call is the same in a variant's library)
// weight_code: the SEC-DED axis of bnn_mi355x_wecc_exposure_campaigns over the weights of layers >= 1 (wecc.h); 0 everywhere else
// weight_interleave: the column interleave of those code words (bnn_mi355x_iwecc_exposure_campaigns; mem_org.h); 0 everywhere else
struct Hardening { int scheme, burst, code = 0, weight_code = 0, weight_interleave = 0; };

static int mem_noise_check(const char *who, const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates, const Hardening &hz,
                           bool base_only) {
  Runtime &r = rt();
  const NetSpec &net = r.spec;
  if (hz.burst < 1 || hz.burst > kMaxBurst) return fail(std::string(who) + ": burst must be 1 ... " + std::to_string(kMaxBurst));
  EccOrg org;
  const std::string e = ecc_layout(net, hz.scheme, hz.code, 0, org);
  if (!e.empty()) return fail(std::string(who) + ": " + e);
  if (!rate_w_q32 || !rate_t_q32 || n_rates != net.nlayers)
    return fail(std::string(who) + ": bad arguments (a rate array missing, or n_rates is not " + std::to_string(net.nlayers) + ": one rate per layer)");
  for (int l = 0; l < net.nlayers; l++)
    if (rate_t_q32[l] != 0 && net.L[l].nthr == 0)
      return fail(std::string(who) + ": layer " + std::to_string(l) + " has no threshold memory (its threshold rate must be 0)");
#ifdef BNN_VARIANT
  if (base_only) return fail("fault injection is not modelled for " BNN_VARIANT " (replicated / interleaved parameter memories); use the base network");
#endif
  if (!ready()) return -1;
  if (r.raw.empty()) return fail("fault injection needs the parameter files (load_parameters), not an imported blob");
  if (r.l1_mfma || r.l1_literal)
    return fail("fault injection is not wired to the BNN_MI355X_L1 comparison forms (the matrix-pipe table is not patched)");
  return 0;
}

// What the host prepares for the runs' copies: the patches of layer 0 of the CNV nets (int8 taps, 24-bit thresholds that
// apply_fault reads back as their integer part, three table forms: drawn and applied here, fault_campaigns' way) and the raw
// 16-bit threshold words of the layers whose threshold rate is not 0, for the threshold kernels.
struct MemNoiseJob {
  size_t stride = 0, spans_off = 0, tab_off[9] = {};
  int nspans = 0;
  std::vector<uint8_t> upload;                  // patch bytes | patch spans | threshold tables
  std::vector<unsigned long long> host_counts;  // [run][layer][2]: the flips the host applied (the plain route)
  // the exposure path: host_counts is [run][epoch][layer][2][2]; the spans are ordered by epoch, epoch t's being
  // span_first[t] ... span_first[t + 1] - 1; k_xmem_noise_t's state of layer l (runs * rows * nthr words) lies at
  // state_off[l] of d_camp, all of them in [state_begin, state_begin + state_bytes)
  std::vector<int> span_first;
  size_t state_off[9] = {}, state_begin = 0, state_bytes = 0;
  // the coded weight route: k_wmem_noise_w's state pairs of layer l (runs * code words of them) at wstate_off[l], inside the
  // same [state_begin, state_begin + state_bytes), so that a full rewrite clears them with the threshold state
  size_t wstate_off[9] = {};
  uint32_t wstate_words[9] = {};  // code words of layer l per run; 0: not coded (or a weight rate of 0)
  // weight_interleave 1: the layer's interleave depth (k_iwmem_noise_w's pairs are physical, in site order); else 0
  uint32_t wdepth[9] = {};
  // the repair route: [run][epoch][layer][2] of the host's layer-0 repairs (words rewritten, words still unlike the loaded ones)
  std::vector<unsigned long long> host_repairs;
};

// Layer 0 of one run through the physical model (mem_org.h): the events of every module applied to `phys` in order, the
// logical memories voted and de-interleaved into raw.w[0] / raw.t[0], the rows whose words now differ from the loaded ones
// marked.  counts: [2: weights, thresholds][2: physical bits flipped, logical bits that differ].
// One state is stepped through the epochs: the events are those of `epoch`, and phys stays as they left it.  Without an
// event nothing but `touched` (cleared) is written: the logical state is the one phys had, which the caller knows.
static int hardened_layer0(const Hardening &hz, unsigned long long seed, const unsigned int rate[2], PhysParams &phys, RawParams &raw,
                           std::vector<char> &touched, unsigned long long counts[4], int epoch) {
  Runtime &r = rt();
  const NetSpec &net = r.spec;
  const LayerSpec &L = net.L[0];
  MemOrg org;
  hardening_layout(net, hz.scheme, 0, org);
  std::vector<PhysFault> ev(256);
  bool any = false;
  for (int target = 0; target < 2; target++) {
    const int ebits = mem_element_bits(L, target);
    for (int m = 0; m < (target ? org.t_modules : org.w_modules); m++) {
      // (one draw where the events fit the buffer: an exposure campaign comes here runs x epochs x modules times)
      const long k = hardened_mem_noise_mask(net, hz.scheme, hz.burst, seed, 0, target, m, rate[target], 0, ev.data(), (long)ev.size(), epoch);
      if (k < 0) return fail("internal: hardened layer-0 draw");
      if ((size_t)k > ev.size()) {
        ev.resize((size_t)k);
        hardened_mem_noise_mask(net, hz.scheme, hz.burst, seed, 0, target, m, rate[target], 0, ev.data(), k, epoch);
      }
      for (long i = 0; i < k; i++) {
        const PhysFault &pf = ev[(size_t)i];
        if (phys_apply(net, hz.scheme, phys, pf) < 0) return fail("internal: hardened layer-0 event outside the memories");
        counts[2 * target] += (unsigned long long)event_width(ebits, hz.burst, pf.f.bit);
        any = true;
      }
    }
  }
  std::fill(touched.begin(), touched.end(), 0);
  if (!any) return 0;
  phys_logical(net, hz.scheme, phys, raw);
  for (int target = 0; target < 2; target++) {
    const int ebits = mem_element_bits(L, target);
    const uint64_t emask = (1ull << ebits) - 1;
    const auto &now = target ? raw.t[0] : raw.w[0];
    const auto &was = target ? r.raw.t[0] : r.raw.w[0];
    for (size_t pe = 0; pe < now.size(); pe++)
      for (size_t i = 0; i < now[pe].size(); i++) {
        const uint64_t d = (now[pe][i] ^ was[pe][i]) & emask;
        if (!d) continue;
        counts[2 * target + 1] += (unsigned long long)__builtin_popcountll(d);
        const size_t ind = target ? i / (size_t)L.nthr : i;  // (apply_fault's row formula)
        touched[(target ? ind : ind / (size_t)(L.fold.wmem / L.fold.tmem)) * (size_t)L.fold.pe + pe] = 1;
      }
  }
  return 0;
}

static void mem_noise_upload(const std::vector<uint8_t> &staging, const std::vector<PatchSpan> &spans, const unsigned int *rth, MemNoiseJob &job);

// The plain route (bnn_mi355x_mem_noise_campaigns, _mem_noise_params): independent single-bit flips of the memories as
// loaded, all of them in place before the first image.  Layer 0 of the CNV nets: mem_noise_mask's flips through apply_fault.
static int mem_noise_prepare(const std::vector<unsigned long long> &seeds, const unsigned int *rw, const unsigned int *rth, MemNoiseJob &job) {
  Runtime &r = rt();
  const NetSpec &net = r.spec;
  const int R = (int)seeds.size(), S = net.nlayers;
  PackedHeader h;
  std::memcpy(&h, r.blob.data(), sizeof(h));
  job.stride = (r.blob.size() + 255) & ~(size_t)255;
  job.host_counts.assign((size_t)R * S * 2, 0);
  std::vector<uint8_t> staging;
  std::vector<PatchSpan> spans;
  if (net.L[0].arith == AR_INT8 && (rw[0] || rth[0])) {
    // ONE working copy of layer 0's memories and of the blob: a run's flips applied in order, the rebuilt rows and tables
    // recorded as its patches, then both restored
    RawParams raw;  // (layer 0's memories alone: nothing else is read here)
    raw.w[0] = r.raw.w[0];
    raw.t[0] = r.raw.t[0];
    std::vector<uint8_t> blob = r.blob;
    const size_t rb = (size_t)h.layer[0].row_dwords * 4, rows_bytes = rb * h.layer[0].rows;
    std::vector<Fault> flips;
    std::vector<char> touched(h.layer[0].rows);
    for (int q = 0; q < R; q++) {
      flips.clear();
      for (int target = 0; target < 2; target++) {
        const uint32_t rate = target ? rth[0] : rw[0];
        const long k = mem_noise_mask(net, seeds[(size_t)q], 0, target, rate, 0, nullptr, 0);
        const size_t at = flips.size();
        flips.resize(at + (size_t)k);
        mem_noise_mask(net, seeds[(size_t)q], 0, target, rate, 0, flips.data() + at, k);
        job.host_counts[((size_t)q * S + 0) * 2 + target] = (unsigned long long)k;
      }
      if (flips.empty()) continue;
      std::fill(touched.begin(), touched.end(), 0);
      for (const Fault &f : flips) {
        const int row = apply_fault(net, raw, f);
        if (row < 0 || row >= (int)h.layer[0].rows) return fail("internal: mem_noise flip outside layer 0");
        touched[(size_t)row] = 1;
      }
      auto add_span = [&](size_t off, size_t bytes) {
        spans.push_back(PatchSpan{(uint64_t)q * job.stride + off, (uint32_t)staging.size(), (uint32_t)bytes});
        staging.insert(staging.end(), blob.begin() + off, blob.begin() + off + bytes);
      };
      for (uint32_t n = 0; n < h.layer[0].rows; n++) {
        if (!touched[n]) continue;
        repack_row_only(net, raw, 0, (int)n, blob);
        add_span(h.layer[0].offset + (size_t)n * rb, rb);
      }
      if (h.l0_mfma_offset) {  // (once per run, not once per row as repack_row would)
        repack_l0_tables(net, raw, blob);
        add_span(h.l0_mfma_offset, kL0MfmaBytes);
      }
      raw.w[0] = r.raw.w[0];
      raw.t[0] = r.raw.t[0];
      std::memcpy(blob.data() + h.layer[0].offset, r.blob.data() + h.layer[0].offset, rows_bytes);
      if (h.l0_mfma_offset) std::memcpy(blob.data() + h.l0_mfma_offset, r.blob.data() + h.l0_mfma_offset, kL0MfmaBytes);
      if (staging.size() > 0xFFFF0000u) return fail("mem_noise: too many layer-0 patches for one call (staging above 4 GB)");
    }
  }
  mem_noise_upload(staging, spans, rth, job);
  return 0;
}

// the upload of a job: patch bytes | patch spans | the raw 16-bit threshold tables of the layers with a threshold rate
static void mem_noise_upload(const std::vector<uint8_t> &staging, const std::vector<PatchSpan> &spans, const unsigned int *rth, MemNoiseJob &job) {
  Runtime &r = rt();
  const NetSpec &net = r.spec;
  const int S = net.nlayers;
  job.nspans = (int)spans.size();
  job.spans_off = (staging.size() + 255) & ~(size_t)255;
  size_t end = job.spans_off + spans.size() * sizeof(PatchSpan);
  for (int l = 0; l < S; l++) {
    const LayerSpec &L = net.L[l];
    if (!rth[l] || L.thr24) continue;
    end = (end + 255) & ~(size_t)255;
    job.tab_off[l] = end;
    end += (size_t)L.mh() * L.nthr * sizeof(uint16_t);
  }
  job.upload.assign(end, 0);
  if (!staging.empty()) std::memcpy(job.upload.data(), staging.data(), staging.size());
  if (!spans.empty()) std::memcpy(job.upload.data() + job.spans_off, spans.data(), spans.size() * sizeof(PatchSpan));
  for (int l = 0; l < S; l++) {
    const LayerSpec &L = net.L[l];
    if (!rth[l] || L.thr24) continue;
    uint16_t *tab = reinterpret_cast<uint16_t *>(job.upload.data() + job.tab_off[l]);
    for (int n = 0; n < L.mh(); n++)
      for (int i = 0; i < L.nthr; i++)
        tab[(size_t)n * L.nthr + i] = (uint16_t)(r.raw.t[l][(size_t)(n % L.fold.pe)][(size_t)(n / L.fold.pe) * L.nthr + i] & 0xFFFF);
  }
}

// R copies of the loaded blob in r.d_copies, `stride` apart, on r.stream
static int replicate_blob(int R, size_t stride) {
  Runtime &r = rt();
  HIP_OK(hipMemcpyAsync(r.d_copies, r.d_blob, r.blob.size(), hipMemcpyDeviceToDevice, r.stream));
  for (size_t have = 1; have < (size_t)R; have *= 2) {  // replicate by doubling
    const size_t c = std::min(have, (size_t)R - have);
    HIP_OK(hipMemcpyAsync(r.d_copies + have * stride, r.d_copies, c * stride, hipMemcpyDeviceToDevice, r.stream));
  }
  return 0;
}

// The plain route, enqueued on r.stream: one copy of the loaded blob per seed in r.d_copies (replicated by doubling), the
// host's layer-0 patches scattered over them, then the upset kernels layer by layer, weights before thresholds.  d_noise
// holds the seeds and, at counts_off, the zeroed [run][layer][2] counters.  `seeds` and `job` must outlive the stream's work.
static int mem_noise_enqueue(const std::vector<unsigned long long> &seeds, const unsigned int *rw, const unsigned int *rth, const MemNoiseJob &job,
                             size_t counts_off) {
  Runtime &r = rt();
  const NetSpec &net = r.spec;
  const int R = (int)seeds.size(), S = net.nlayers;
  PackedHeader h;
  std::memcpy(&h, r.blob.data(), sizeof(h));
  const size_t stride = job.stride;
  if (r.d_copies.grow((size_t)R * stride) || r.d_camp.grow(job.upload.size() + 256) ||
      r.d_noise.grow(counts_off + (size_t)R * S * 2 * 8))
    return -1;
  const unsigned long long *const d_seeds = reinterpret_cast<const unsigned long long *>(r.d_noise.get());
  unsigned long long *const d_counts = reinterpret_cast<unsigned long long *>(r.d_noise + counts_off);
  HIP_OK(hipMemcpyAsync(r.d_noise, seeds.data(), (size_t)R * 8, hipMemcpyHostToDevice, r.stream));
  HIP_OK(hipMemsetAsync(d_counts, 0, (size_t)R * S * 2 * 8, r.stream));
  if (replicate_blob(R, stride)) return -1;
  if (!job.upload.empty()) HIP_OK(hipMemcpyAsync(r.d_camp, job.upload.data(), job.upload.size(), hipMemcpyHostToDevice, r.stream));
  hipError_t e = scatter_patches(r.d_camp, reinterpret_cast<const PatchSpan *>(r.d_camp + job.spans_off), job.nspans, r.d_copies, r.stream);
  for (int l = 0; l < S && e == hipSuccess; l++) {
    const LayerSpec &L = net.L[l];
    if (L.arith == AR_INT8) continue;  // (the host's part)
    const MemNoiseLayer ml{h.layer[l].offset, h.layer[l].row_dwords, h.layer[l].rows, h.layer[l].kw, (uint32_t)L.fold.pe, (uint32_t)L.fold.tmem, (uint32_t)l};
    e = mem_noise_w(r.d_copies, stride, R, d_seeds, ml, L.arith == AR_TT, rw[l], d_counts, S, r.stream);
    // the loaded parameters hold -2 rows already: a flip may have removed the last -2 of a row
    if (e == hipSuccess && L.arith == AR_TT && rw[l] && r.two_rows > 0) e = mem_noise_flags(r.d_copies, stride, R, ml, r.stream);
    if (e == hipSuccess && rth[l])
      e = mem_noise_t(r.d_copies, stride, R, d_seeds, ml, L.nthr, L.arith, L.signed_bb, reinterpret_cast<const uint16_t *>(r.d_camp + job.tab_off[l]),
                      rth[l], d_counts, S, r.stream);
  }
  if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
  return 0;
}

// ---- the exposure path: upsets of a memory organisation that accumulate over epochs, with scrubbing (the model: mem_org.h) --
// The hardened one-shot campaign (bnn_mi355x_hardened_mem_noise_campaigns) is one epoch that is never scrubbed: epoch 0's
// tag is kMemNoiseTag, and its upsets meet zeroed state.

// longs: the counters per (run, epoch, layer) -- 4, or 6 on the coded route (the ecc entry points, with code 0 as well), 8
// on the repair route (with repair_every 0 as well), 12 on the coded weight routes: which blocks ExposureCounters has
// repair_every: the repair scrub of mem_org.h ("repair scrubs"); 0 never
struct Exposure { int epoch_images, scrub_every, longs = 4, repair_every = 0; };

// The counter region of the exposure path, on the device (from counts_off of d_noise on) and read back: up to four blocks
// one behind the other, each [run][epoch][layer][width(b)] longs.  A family with `longs` counters has the blocks whose
// columns lie below that; bnn_mi355x_last_*_counts hands out [run][epoch][layer][longs], block b from column(b) on.
struct ExposureCounters {
  enum Block {
    COUNTS,   // [2: weights, thresholds][2: physical bits flipped, logical bits that differ]: the upset kernels' and the host's
    STATUS,   // threshold words corrected, detected as uncorrectable (k_emem_noise_t)
    REPAIRS,  // words a repair rewrote, words still unlike the loaded ones after it (k_repair_state and the host)
    WSTATUS,  // weight code words corrected, detected, rewritten, still unlike (k_wmem_noise_w / k_iwmem_noise_w, k_wrepair_state / k_iwrepair_state)
    BLOCKS
  };
  size_t R, E, S;
  int longs;
  static size_t width(int b) { return b == STATUS || b == REPAIRS ? 2 : 4; }
  static size_t column(int b) { return b == COUNTS ? 0 : b == STATUS ? 4 : b == REPAIRS ? 6 : 8; }
  bool has(int b) const { return (size_t)longs > column(b); }
  size_t cells() const { return R * E * S; }
  size_t offset(int b) const { return cells() * column(b); }    // of the block, in longs
  size_t run_stride(int b) const { return E * S * width(b); }  // from a run's counters to the next run's, in longs
  size_t bytes() const { return cells() * (size_t)longs * 8; }
  // epoch t of run 0 in block b of the region at `region`; nullptr for a block the family has not
  unsigned long long *epoch(uint8_t *region, int b, int t) const {
    return has(b) ? reinterpret_cast<unsigned long long *>(region) + offset(b) + (size_t)t * S * width(b) : nullptr;
  }
};

static bool exposure_scrubs(const Exposure &ex, int t) { return exposure_rewrites(t, ex.scrub_every); }
static bool exposure_repairs(const Exposure &ex, int t) { return exposure_repairs(t, ex.scrub_every, ex.repair_every); }

// What the host prepares for E epochs.  Layer 0 of the CNV nets: one persistent physical working state per run is stepped
// through the epochs by hardened_layer0, scrubs included (the draw is deterministic, so all of it is known before anything
// is enqueued); the rows and tables an epoch changes become that epoch's patches.  A row is rebuilt where its words differ from the loaded
// ones now or did so after the epoch before (it may have returned to them).  Then the threshold tables (mem_noise_upload),
// and the layout of the threshold state.
static int exposure_prepare(const char *who, const std::vector<unsigned long long> &seeds, const unsigned int *rw, const unsigned int *rth,
                            const ExposureCounters &cl, const Exposure &ex, const Hardening &hz, MemNoiseJob &job) {
  Runtime &r = rt();
  const NetSpec &net = r.spec;
  const int R = (int)seeds.size(), E = (int)cl.E, S = net.nlayers;
  PackedHeader h;
  std::memcpy(&h, r.blob.data(), sizeof(h));
  job.stride = (r.blob.size() + 255) & ~(size_t)255;
  job.host_counts.assign(cl.cells() * cl.width(cl.COUNTS), 0);
  job.host_repairs.assign(cl.has(cl.REPAIRS) ? cl.cells() * cl.width(cl.REPAIRS) : 0, 0);
  std::vector<uint8_t> staging;
  std::vector<std::vector<PatchSpan>> by_epoch((size_t)E);
  if (net.L[0].arith == AR_INT8 && (rw[0] || rth[0])) {
    RawParams raw;  // (layer 0's memories alone: nothing else is read here)
    raw.w[0] = r.raw.w[0];
    raw.t[0] = r.raw.t[0];
    // the rows and tables are packed into a working blob and copied out: every span is rebuilt from `raw` in full, so what
    // an earlier epoch or run left in the blob is never uploaded
    std::vector<uint8_t> blob = r.blob;
    const size_t rb = (size_t)h.layer[0].row_dwords * 4;
    std::vector<char> touched(h.layer[0].rows), before(h.layer[0].rows);
    PhysParams loaded, phys;
    phys_load(net, hz.scheme, r.raw, 0, 1, loaded);
    const unsigned int rate[2] = {rw[0], rth[0]};
    for (int q = 0; q < R; q++) {
      phys = loaded;
      std::fill(before.begin(), before.end(), 0);
      for (int t = 0; t < E; t++) {
        unsigned long long *const counts = &job.host_counts[(((size_t)q * E + t) * S + 0) * 4];
        const bool scrub = exposure_scrubs(ex, t);
        if (scrub) {  // (the copies on the device return to the loaded blob as well)
          phys = loaded;
          std::fill(before.begin(), before.end(), 0);
        } else if (exposure_repairs(ex, t)) {
          // a repair: the modules of layer 0 voted and written back.  The delivered rows do not change: no patch
          long rc[1][2];
          phys_repair(net, hz.scheme, hz.code, phys, 0, 1, rc, &loaded);
          job.host_repairs[(((size_t)q * E + t) * S + 0) * 2] = (unsigned long long)rc[0][0];
          job.host_repairs[(((size_t)q * E + t) * S + 0) * 2 + 1] = (unsigned long long)rc[0][1];
        }
        if (hardened_layer0(hz, seeds[(size_t)q], rate, phys, raw, touched, counts, t)) return -1;
        if (counts[0] + counts[2] == 0) {  // no event: nothing to patch; without a scrub the logical state is the last epoch's
          if (!scrub && t > 0) {
            counts[1] = counts[1 - S * 4];
            counts[3] = counts[3 - S * 4];
          }
          continue;
        }
        auto add_span = [&](size_t off, size_t bytes) {
          by_epoch[(size_t)t].push_back(PatchSpan{(uint64_t)q * job.stride + off, (uint32_t)staging.size(), (uint32_t)bytes});
          staging.insert(staging.end(), blob.begin() + off, blob.begin() + off + bytes);
        };
        bool rebuilt = false;
        for (uint32_t n = 0; n < h.layer[0].rows; n++) {
          if (!touched[n] && !before[n]) continue;
          repack_row_only(net, raw, 0, (int)n, blob);
          add_span(h.layer[0].offset + (size_t)n * rb, rb);
          rebuilt = true;
        }
        if (rebuilt && h.l0_mfma_offset) {  // (once per epoch, not once per row as repack_row would)
          repack_l0_tables(net, raw, blob);
          add_span(h.l0_mfma_offset, kL0MfmaBytes);
        }
        before = touched;
        if (staging.size() > 0xFFFF0000u) return fail(std::string(who) + ": too many layer-0 patches for one call (staging above 4 GB)");
      }
    }
  }
  std::vector<PatchSpan> spans;
  job.span_first.assign((size_t)E + 1, 0);
  for (int t = 0; t < E; t++) {
    spans.insert(spans.end(), by_epoch[(size_t)t].begin(), by_epoch[(size_t)t].end());
    job.span_first[(size_t)t + 1] = (int)spans.size();
  }
  mem_noise_upload(staging, spans, rth, job);
  size_t end = (job.upload.size() + 255) & ~(size_t)255;
  job.state_begin = end;
  for (int l = 0; l < S; l++) {
    const LayerSpec &L = net.L[l];
    if (!rth[l] || L.thr24) continue;
    job.state_off[l] = end;
    end += (((size_t)R * L.mh() * L.nthr * 8) + 255) & ~(size_t)255;
  }
  for (int l = 0; l < S; l++) {  // (the coded weight memories: a pair of longs per code word)
    const int cwpp = wecc_words_per_pe(net, hz.weight_code, l);
    if (!rw[l] || !cwpp) continue;
    job.wstate_off[l] = end;
    job.wstate_words[l] = (uint32_t)cwpp * (uint32_t)net.L[l].fold.pe;
    if (hz.weight_interleave) job.wdepth[l] = (uint32_t)wecc_depth(net, hz.weight_code, hz.weight_interleave, l);
    end += (((size_t)R * job.wstate_words[l] * 16) + 255) & ~(size_t)255;
  }
  job.state_bytes = end - job.state_begin;
  return 0;
}

// Enqueues on r.stream what comes before epoch 0: the seeds, the zeroed counter region `cl` at counts_off of d_noise, the
// runs' copies of the loaded blob, the job's upload and the zeroed threshold state.
static int exposure_begin(const std::vector<unsigned long long> &seeds, const MemNoiseJob &job, size_t counts_off, const ExposureCounters &cl) {
  Runtime &r = rt();
  const int R = (int)seeds.size();
  if (r.d_copies.grow((size_t)R * job.stride) || r.d_camp.grow(job.state_begin + job.state_bytes + 256) ||
      r.d_noise.grow(counts_off + cl.bytes()))
    return -1;
  HIP_OK(hipMemcpyAsync(r.d_noise, seeds.data(), (size_t)R * 8, hipMemcpyHostToDevice, r.stream));
  HIP_OK(hipMemsetAsync(r.d_noise + counts_off, 0, cl.bytes(), r.stream));
  if (replicate_blob(R, job.stride)) return -1;
  if (!job.upload.empty()) HIP_OK(hipMemcpyAsync(r.d_camp, job.upload.data(), job.upload.size(), hipMemcpyHostToDevice, r.stream));
  if (job.state_bytes) HIP_OK(hipMemsetAsync(r.d_camp + job.state_begin, 0, job.state_bytes, r.stream));
  return 0;
}

// Enqueues epoch t: the scrub where one is due (the copies restored by the same doubling copy, the state cleared) or
// else the repair where one is due (ONE launch of k_repair_state over the state of every layer with redundancy), the
// host's layer-0 patches of the epoch, then the upset kernels layer by layer, weights before thresholds.
static int exposure_epoch(int t, const unsigned int *rw, const unsigned int *rth, const MemNoiseJob &job, size_t counts_off,
                          const ExposureCounters &cl, const Exposure &ex, const Hardening &hz) {
  Runtime &r = rt();
  const NetSpec &net = r.spec;
  const int R = (int)cl.R, S = net.nlayers;
  PackedHeader h;
  std::memcpy(&h, r.blob.data(), sizeof(h));
  const size_t stride = job.stride;
  const unsigned long long *const d_seeds = reinterpret_cast<const unsigned long long *>(r.d_noise.get());
  // epoch t of every block (a kernel whose block the family has not is never launched)
  uint8_t *const region = r.d_noise + counts_off;
  unsigned long long *const d_counts = cl.epoch(region, cl.COUNTS, t), *const d_ecc = cl.epoch(region, cl.STATUS, t),
                           *const d_rep = cl.epoch(region, cl.REPAIRS, t), *const d_wst = cl.epoch(region, cl.WSTATUS, t);
  const size_t run_stride = cl.run_stride(cl.COUNTS);
  if (exposure_scrubs(ex, t)) {
    if (replicate_blob(R, stride)) return -1;
    if (job.state_bytes) HIP_OK(hipMemsetAsync(r.d_camp + job.state_begin, 0, job.state_bytes, r.stream));
  } else if (exposure_repairs(ex, t) && cl.has(cl.REPAIRS) && job.state_bytes) {
    RepairTable tab{};
    int entries = 0;
    for (int l = 0; l < S; l++) {
      const LayerSpec &L = net.L[l];
      if (!rth[l] || L.thr24 || L.arith == AR_INT8) continue;  // (no state: nothing to repair)
      EccOrg eo{MemOrg{1, 1, 0}, 0};
      ecc_layout(net, hz.scheme, hz.code, l, eo);
      const uint32_t kind = eo.check_bits ? RK_CODED : eo.org.t_modules == 3 ? RK_TMR : RK_SKIP;
      if (kind != RK_SKIP) tab.e[entries++] = RepairEntry{(unsigned long long)job.state_off[l], h.layer[l].rows * (uint32_t)L.nthr, kind, (uint32_t)l, 0};
    }
    const hipError_t re = repair_state(r.d_camp, tab, entries, R, d_rep, cl.run_stride(cl.REPAIRS), r.stream);
    if (re != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(re));
    // the coded weight memories: one more launch over their state pairs
    RepairTable wtab{};
    int wentries = 0;
    for (int l = 0; l < S; l++)
      if (job.wstate_words[l])
        wtab.e[wentries++] = RepairEntry{(unsigned long long)job.wstate_off[l], job.wstate_words[l], RK_CODED, (uint32_t)l, job.wdepth[l]};
    if (wentries) {
      // (weight_interleave 1: every coded layer's pairs are physical ones, so the interleaved repair goes INSTEAD)
      const hipError_t we = hz.weight_interleave ? iwrepair_state(r.d_camp, wtab, wentries, R, d_wst, cl.run_stride(cl.WSTATUS), r.stream)
                                                 : wrepair_state(r.d_camp, wtab, wentries, R, d_wst, cl.run_stride(cl.WSTATUS), r.stream);
      if (we != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(we));
    }
  }
  const int s0 = job.span_first[(size_t)t], s1 = job.span_first[(size_t)t + 1];
  hipError_t e = scatter_patches(r.d_camp, reinterpret_cast<const PatchSpan *>(r.d_camp + job.spans_off) + s0, s1 - s0, r.d_copies, r.stream);
  for (int l = 0; l < S && e == hipSuccess; l++) {
    const LayerSpec &L = net.L[l];
    if (L.arith == AR_INT8) continue;  // (the host's part)
    const MemNoiseLayer ml{h.layer[l].offset, h.layer[l].row_dwords, h.layer[l].rows, h.layer[l].kw, (uint32_t)L.fold.pe, (uint32_t)L.fold.tmem, (uint32_t)l};
    EccOrg eo{MemOrg{1, 1, 0}, 0};
    ecc_layout(net, hz.scheme, hz.code, l, eo);  // (checked by mem_noise_check; weights of a layer >= 1 have one module)
    const MemOrg &org = eo.org;
    if (job.wstate_words[l]) {
      // a coded weight memory (weight_code 1 comes by the 12-long route alone, which has the WSTATUS block)
      if (job.wdepth[l])
        e = iwmem_noise_w(r.d_copies, stride, R, d_seeds, ml, L.arith == AR_TT, mem_element_bits(L, 0), hz.burst, (int)job.wdepth[l], rw[l], t,
                          static_cast<const uint8_t *>(r.d_blob), reinterpret_cast<unsigned long long *>(r.d_camp + job.wstate_off[l]), d_counts,
                          run_stride, d_wst, cl.run_stride(cl.WSTATUS), r.stream);
      else
        e = wmem_noise_w(r.d_copies, stride, R, d_seeds, ml, L.arith == AR_TT, mem_element_bits(L, 0), hz.burst, rw[l], t,
                         static_cast<const uint8_t *>(r.d_blob), reinterpret_cast<unsigned long long *>(r.d_camp + job.wstate_off[l]), d_counts,
                         run_stride, d_wst, cl.run_stride(cl.WSTATUS), r.stream);
    } else
      e = xmem_noise_w(r.d_copies, stride, R, d_seeds, ml, L.arith == AR_TT, mem_element_bits(L, 0), hz.burst, rw[l], t,
                       static_cast<const uint8_t *>(r.d_blob), d_counts, run_stride, r.stream);
    // a flip may have removed the last -2 of a row (the loaded parameters may hold -2 rows, and so may an earlier epoch's state)
    if (e == hipSuccess && L.arith == AR_TT && rw[l] && (r.two_rows > 0 || t > 0)) e = mem_noise_flags(r.d_copies, stride, R, ml, r.stream);
    if (e == hipSuccess && rth[l] && eo.check_bits) {
      // a coded layer (code 1 comes by the routes of 6 longs and more alone, which have the STATUS block)
      e = emem_noise_t(r.d_copies, stride, R, d_seeds, ml, L.nthr, L.arith, L.signed_bb, reinterpret_cast<const uint16_t *>(r.d_camp + job.tab_off[l]),
                       org.t_interleave, hz.burst, rth[l], t, reinterpret_cast<unsigned long long *>(r.d_camp + job.state_off[l]), d_counts,
                       run_stride, d_ecc, cl.run_stride(cl.STATUS), r.stream);
    } else if (e == hipSuccess && rth[l])
      e = xmem_noise_t(r.d_copies, stride, R, d_seeds, ml, L.nthr, L.arith, L.signed_bb, reinterpret_cast<const uint16_t *>(r.d_camp + job.tab_off[l]),
                       org.t_modules, org.t_interleave, hz.burst, rth[l], t, reinterpret_cast<unsigned long long *>(r.d_camp + job.state_off[l]),
                       d_counts, run_stride, r.stream);
  }
  if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
  return 0;
}

// What is an entry point's own: everything else is the same call.
struct MemNoiseEntry {
  const char *who;                                  // its name in every refusal
  std::vector<long> Runtime::*counts;               // its bnn_mi355x_last_*_counts
  std::vector<unsigned long long> Runtime::*seeds;  // and bnn_mi355x_last_*_seeds
  bool one_epoch = false;      // no epoch arguments: the whole file is ONE epoch (an empty file as well), never scrubbed
  bool base_only = false;      // a variant's library refuses it (mem_noise_check)
  bool plain = false;          // the plain route (mem_noise_prepare, mem_noise_enqueue): its counters are [run][layer][2]
  bool file_first = false;     // the file is opened and its epochs are counted before mem_noise_check
};

// Random upsets of the parameter memories, many runs in one call.  Every run gets a copy of the loaded blob in HBM; the images
// go epoch by epoch, each epoch's scrub and upsets enqueued in front of its pairs and applied to the copies in place
// (exposure_epoch; the plain route: all of it in front of the one epoch's pairs, mem_noise_enqueue); an epoch's (run, image)
// pairs go in run-major order, in groups of at most one activation workspace, through the multi-run stages with the copy
// stride: act_noise_campaigns' grouping with fault_campaigns' copies.  kMaxRuns copies are what fault_campaigns holds as
// well, so a call's runs always fit.  The counters are ExposureCounters' blocks; the plain route's are [run][layer][2].
static int *mem_noise_campaigns_impl(const MemNoiseEntry &en, const Hardening &hz, const Exposure &ex, const char *path, int number_class,
                                     int num_runs, unsigned long long seed, const unsigned int *rate_w_q32, const unsigned int *rate_t_q32,
                                     int n_rates, int *image_number, float *usecPerImage) {
  Runtime &r = rt();
  const NetSpec &net = r.spec;
  const char *const who = en.who;
  std::vector<long> &last_counts = r.*en.counts;
  std::vector<unsigned long long> &last_seeds = r.*en.seeds;
  last_counts.clear();
  last_seeds.clear();
  const int S = net.nlayers;
  if (!en.one_epoch && (ex.epoch_images < 1 || ex.scrub_every < 0)) {
    fail(std::string(who) + ": epoch_images must be at least 1 and scrub_every must not be negative (0: never scrub)");
    return nullptr;
  }
  if (ex.repair_every < 0) {
    fail(std::string(who) + ": repair_every must not be negative (0: never repair)");
    return nullptr;
  }
  if (!path) {
    fail(std::string(who) + ": bad arguments (path missing)");
    return nullptr;
  }
  if (num_runs < 1 || num_runs > kMaxRuns) {
    fail(std::string(who) + ": num_runs must be 1 ... " + std::to_string(kMaxRuns));
    return nullptr;
  }
  const int R = num_runs;
  if (seed != 0 && 0ull - (uint64_t)seed < (uint64_t)R) {
    fail(std::string(who) + ": seed + run wraps to 0 for a run (0 seeds from std::random_device)");
    return nullptr;
  }
  ImageFile f;
  // the epochs a file implies, refused where they or their counters are too many; `false` once that is known not to be so
  auto too_many_epochs = [&]() -> bool {
    const long long epochs = en.one_epoch ? 1 : ((long long)f.n + ex.epoch_images - 1) / ex.epoch_images;
    if (epochs <= kMaxEpochs && (unsigned long long)R * (unsigned long long)epochs * S * (unsigned)ex.longs <= 0x7FFFFFFFull) return false;
    fail(std::string(who) + ": " + std::to_string(epochs) + " epochs: at most " + std::to_string(kMaxEpochs) +
         ", and num_runs * epochs * layers * " + std::to_string(ex.longs) + " counters must stay below 2^31");
    return true;
  };
  // (file_first, the repair entry point: every argument is refused before a device is looked for -- mem_noise_check ends with
  // ready(), the first thing that may touch one -- and the file's size is known without a device; the others keep the order they had)
  if (en.file_first && (open_image_file(path, f) || too_many_epochs())) return nullptr;
  if (mem_noise_check(who, rate_w_q32, rate_t_q32, n_rates, hz, en.base_only)) return nullptr;
  if (!en.file_first && open_image_file(path, f)) return nullptr;
  const int n = (int)f.n;
  const size_t total = (size_t)R * n;
  const bool cnv = net.is_cnv;
  const int ei = en.one_epoch ? std::max(n, 1) : ex.epoch_images;  // images per epoch
  if (!en.file_first && too_many_epochs()) return nullptr;
  const int E = en.one_epoch ? 1 : (int)(((long long)n + ei - 1) / ei);
  std::vector<unsigned long long> seeds((size_t)R);
  {
    std::random_device rd;
    for (int q = 0; q < R; q++) {
      unsigned long long k = seed ? seed + (unsigned long long)q : 0;  // (seed 0: every run from std::random_device, never 0)
      while (k == 0) k = ((unsigned long long)rd() << 32) | rd();
      seeds[(size_t)q] = k;
    }
  }
  bool any = false, tt = false;
  for (int l = 0; l < S; l++) {
    any = any || rate_w_q32[l] || rate_t_q32[l];
    tt = tt || (rate_w_q32[l] && net.L[l].arith == AR_TT);
  }
  int *result = new (std::nothrow) int[total + 1];
  if (!result) { fail("out of memory"); return nullptr; }
  const ExposureCounters cl{(size_t)R, (size_t)E, (size_t)S, ex.longs};
  std::vector<unsigned long long> counts(en.plain ? (size_t)R * S * 2 : cl.bytes() / 8, 0);  // the counters as the device holds them
  MemNoiseJob job;
  double device_us = 0.0;
  auto run = [&]() -> int {
    if (n == 0) return 0;
    if (any && (en.plain ? mem_noise_prepare(seeds, rate_w_q32, rate_t_q32, job) : exposure_prepare(who, seeds, rate_w_q32, rate_t_q32, cl, ex, hz, job)))
      return -1;
    size_t cap = std::min<size_t>(kMaxChunk, total);  // pairs per group: the activation workspace
    if (const char *e = std::getenv("BNN_MI355X_NOISE_GROUP")) {  // tests: many small groups
      const long long v = std::atoll(e);
      if (v > 0) cap = std::min<size_t>(cap, (size_t)v);
    }
    // the records of every group: a run's images of one epoch, cut at the group's end; the epochs one after the other
    struct Group { size_t seg0; int nsegs, max_len, total, epoch; };
    std::vector<MultiSeg> segs;
    std::vector<Group> groups;
    for (int t = 0; t < E; t++) {
      const int i0 = t * ei, len = std::min(n, i0 + ei) - i0;  // (t * ei < n)
      const size_t pairs = (size_t)R * len;
      for (size_t p0 = 0; p0 < pairs; p0 += cap) {
        const size_t p1 = std::min(pairs, p0 + cap);
        Group g{segs.size(), 0, 0, 0, t};
        for (size_t p = p0; p < p1;) {
          const int q = (int)(p / (size_t)len), i = (int)(p % (size_t)len), m = (int)std::min<size_t>((size_t)(len - i), p1 - p);
          segs.push_back(MultiSeg{q, i0 + i, g.total, m});
          g.nsegs++;
          g.total += m;
          g.max_len = std::max(g.max_len, m);
          p += (size_t)m;
        }
        groups.push_back(g);
      }
    }
    PackedHeader h;
    std::memcpy(&h, r.blob.data(), sizeof(h));
    const bool tab = h.l0_mfma_offset && r.l0_mfma;
    const size_t counts_off = ((size_t)R * 8 + 255) & ~(size_t)255;
    if (load_file_resident(f, n) || reserve((int)cap)) return -1;
    if (r.d_sw_segs.grow(segs.size() * sizeof(MultiSeg)) ||
        r.d_camp_res.grow(total * (cnv ? sizeof(int32_t) : sizeof(uint64_t))))
      return -1;
    std::vector<uint64_t> w;  // (LFC: raw words, decoded on the host)
    if (!cnv) w.resize(total);
    DrainOnFailure drain;  // (declared after the host buffers the queued copies read or write)
    if (settle_handover(r.stream)) return -1;
    while (r.time_events.size() < 2) {
      hipEvent_t e;
      HIP_OK(hipEventCreateWithFlags(&e, kTimeEventFlags));
      r.time_events.push_back(e);
    }
    // -- all of it on one stream, one wait at the end
    HIP_OK(hipEventRecord(r.time_events[0], r.stream));
    if (any && (en.plain ? mem_noise_enqueue(seeds, rate_w_q32, rate_t_q32, job, counts_off) : exposure_begin(seeds, job, counts_off, cl)))
      return -1;
    // (all rates 0: no copy is made, every run reads the loaded blob)
    const uint8_t *const base = any ? r.d_copies : static_cast<const uint8_t *>(r.d_blob);
    const MultiSeg *const d_segs = reinterpret_cast<const MultiSeg *>(r.d_sw_segs.get());
    HIP_OK(hipMemcpyAsync(r.d_sw_segs, segs.data(), segs.size() * sizeof(MultiSeg), hipMemcpyHostToDevice, r.stream));
    int entered = -1;  // the last epoch whose scrub and upsets are in the stream
    for (const Group &g : groups) {
      for (; !en.plain && any && entered < g.epoch; entered++)
        if (exposure_epoch(entered + 1, rate_w_q32, rate_t_q32, job, counts_off, cl, ex, hz)) return -1;
      MultiLaunch a{};
      a.images = r.d_all;
      a.segs = d_segs + g.seg0;
      a.nsegs = g.nsegs; a.max_len = g.max_len; a.total = g.total; a.n = n;
      a.buf0 = r.buf0; a.buf1 = r.buf1;
      for (int k = 0; k < S; k++) a.rows[k] = reinterpret_cast<const uint32_t *>(base + h.layer[k].offset);
      a.l0_mfma = tab ? base + h.l0_mfma_offset : nullptr;
      a.stride = any ? job.stride : 0;
      // (reading the flags back only to decide this would cost a host wait: the -2-aware instantiations are exact on rows without)
      a.has_two = r.two_rows > 0 || tt;
      a.classes = reinterpret_cast<int32_t *>(r.d_camp_res.get());
      a.words = reinterpret_cast<uint64_t *>(r.d_camp_res.get());
      a.number_class = number_class;
      a.stream = r.stream;
      const hipError_t e = cnv ? run_cnv_multi(net.id, a) : run_lfc_multi(net.id, a);
      if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
    }
    HIP_OK(hipEventRecord(r.time_events[1], r.stream));
    if (any) HIP_OK(hipMemcpyAsync(counts.data(), r.d_noise + counts_off, counts.size() * 8, hipMemcpyDeviceToHost, r.stream));
    if (cnv) HIP_OK(hipMemcpyAsync(result, r.d_camp_res, total * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
    else HIP_OK(hipMemcpyAsync(w.data(), r.d_camp_res, total * sizeof(uint64_t), hipMemcpyDeviceToHost, r.stream));
    HIP_OK(hipStreamSynchronize(r.stream));
    for (size_t i = 0; !cnv && i < total; i++) result[i] = lfc_class_batched(w[i], number_class);
    // (the host's layer-0 part, in the shape of the block it goes to)
    for (size_t i = 0; i < job.host_counts.size(); i++) counts[i] += job.host_counts[i];
    for (size_t i = 0; i < job.host_repairs.size(); i++) counts[cl.offset(cl.REPAIRS) + i] += job.host_repairs[i];
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, r.time_events[0], r.time_events[1]));
    drain.ok();
    device_us = ms * 1000.0;
    return 0;
  };
  if (run() < 0) {
    delete[] result;
    return nullptr;
  }
  // the plain route's [run][layer][2] as they are; else the blocks side by side, [run][epoch][layer][longs]
  if (en.plain) {
    last_counts.assign(counts.begin(), counts.end());
  } else {
    last_counts.resize(counts.size());
    long *out = last_counts.data();  // (one pass in the order it is written: a cell's blocks follow each other by column)
    for (size_t c = 0; c < cl.cells(); c++)
      for (int b = 0; b < cl.BLOCKS && cl.has(b); b++) {
        const unsigned long long *const from = counts.data() + cl.offset(b) + c * cl.width(b);
        for (size_t j = 0; j < cl.width(b); j++) *out++ = (long)from[j];
      }
  }
  last_seeds = std::move(seeds);
  if (image_number) *image_number = n;
  if (usecPerImage) *usecPerImage = total ? (float)(device_us / (double)total) : 0.f;
  return result;
}

int *bnn_mi355x_mem_noise_campaigns(const char *path, int number_class, int num_runs, unsigned long long seed,
                                    const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates, int *image_number,
                                    float *usecPerImage) {
  // independent single-bit flips of the memories as loaded (no scheme, burst 1), by the plain route
  const MemNoiseEntry en{"mem_noise_campaigns", &Runtime::mem_noise_counts, &Runtime::mem_noise_seeds, true, true, true};
  return mem_noise_campaigns_impl(en, Hardening{HS_NONE, 1}, Exposure{0, 0}, path, number_class, num_runs, seed, rate_w_q32, rate_t_q32, n_rates,
                                  image_number, usecPerImage);
}

int bnn_mi355x_last_mem_noise_counts(long *flips, int cap) { return copy_out(rt().mem_noise_counts, flips, cap); }

int bnn_mi355x_last_mem_noise_seeds(unsigned long long *seeds, int cap) { return copy_out(rt().mem_noise_seeds, seeds, cap); }

long bnn_mi355x_mem_noise_mask(unsigned long long run_seed, int layer, int target, unsigned int rate_q32, long first, int *records,
                               int cap_records) {
  const NetSpec &net = rt().spec;
  if (mem_noise_sites(net, layer, target) < 0 || first < 0)
    return fail("mem_noise_mask: bad layer (0 ... " + std::to_string(net.nlayers - 1) + "), target (0 weights, 1 thresholds) or first");
  const long total = mem_noise_mask(net, run_seed, layer, target, rate_q32, 0, nullptr, 0);
  if (records && cap_records > 0 && first < total) {
    std::vector<Fault> v((size_t)std::min<long>(cap_records, total - first));
    mem_noise_mask(net, run_seed, layer, target, rate_q32, first, v.data(), (long)v.size());
    for (size_t i = 0; i < v.size(); i++) put_record(v[i], records + i * 8);
  }
  return total;
}

size_t bnn_mi355x_mem_noise_params(unsigned long long run_seed, const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates,
                                   void *dst, size_t cap) {
  const char *const who = "mem_noise_params";
  Runtime &r = rt();
  if (mem_noise_check(who, rate_w_q32, rate_t_q32, n_rates, Hardening{HS_NONE, 1}, true)) return 0;
  if (!dst) return r.blob.size();
  if (cap < r.blob.size()) { fail(std::string(who) + ": destination too small"); return 0; }
  const std::vector<unsigned long long> seeds(1, run_seed);
  MemNoiseJob job;
  auto run = [&]() -> int {
    if (mem_noise_prepare(seeds, rate_w_q32, rate_t_q32, job)) return -1;
    DrainOnFailure drain;  // (declared after the host buffers the queued copies read or write)
    if (settle_handover(r.stream)) return -1;
    if (mem_noise_enqueue(seeds, rate_w_q32, rate_t_q32, job, 256)) return -1;
    HIP_OK(hipMemcpyAsync(dst, r.d_copies, r.blob.size(), hipMemcpyDeviceToHost, r.stream));
    HIP_OK(hipStreamSynchronize(r.stream));
    drain.ok();
    return 0;
  };
  return run() < 0 ? 0 : r.blob.size();
}

// ---- hardened memory schemes in the memory upset campaigns (the model: mem_org.h) ------------------------------------------

int bnn_mi355x_hardening_scheme(void) { return hardening_scheme_of(bnn_mi355x_network()); }

int bnn_mi355x_hardening_layout(int scheme, int layer, int out[3]) {
  MemOrg org;
  const std::string e = hardening_layout(rt().spec, scheme, layer, org);
  if (!e.empty()) return fail("hardening_layout: " + e);
  if (out) { out[0] = org.w_modules; out[1] = org.t_modules; out[2] = org.t_interleave; }
  return 0;
}

int bnn_mi355x_hardened_site(int scheme, int layer, int target, int ind, int bit, int *p_ind, int *p_bit) {
  const NetSpec &net = rt().spec;
  MemOrg org;
  const std::string e = hardening_layout(net, scheme, layer, org);
  if (!e.empty()) return fail("hardened_site: " + e);
  const LayerSpec &L = net.L[layer];
  const int ebits = (target == 0 || target == 1) ? mem_element_bits(L, target) : 0;
  if (ebits == 0 || ind < 0 || ind >= (target ? L.fold.tmem : L.fold.wmem) || bit < 0 || bit >= ebits)
    return fail("hardened_site: target (0 weights, 1 thresholds of a layer that has some), ind or bit outside the memory");
  int pi = ind, pb = bit;
  if (target == 1) interleave_site(org.t_interleave, ebits, L.fold.tmem, ind, bit, &pi, &pb);
  if (p_ind) *p_ind = pi;
  if (p_bit) *p_bit = pb;
  return 0;
}

// The mask entry points of the physical organisations: the layout checked, the events of one (run seed, epoch, layer, target,
// module) counted, those from `first` on drawn and written as 9-int records.  epochs false: an entry point without epochs
// passes epoch 0, and its refusal does not speak of one.
static long phys_noise_mask(const std::string &who, const Hardening &hz, unsigned long long run_seed, bool epochs, int epoch, int layer, int target,
                            int module, unsigned int rate_q32, long first, int *records, int cap_records) {
  const NetSpec &net = rt().spec;
  EccOrg eo;
  const std::string e = ecc_layout(net, hz.scheme, hz.code, layer, eo);
  if (!e.empty()) return fail(who + ": " + e);
  const long total = first < 0 ? -1
                               : hardened_mem_noise_mask(net, hz.scheme, hz.burst, run_seed, layer, target, module, rate_q32, 0, nullptr, 0, epoch, hz.code,
                                                         hz.weight_code);
  if (total < 0)
    return fail(who + ": bad burst (1 ... " + std::to_string(kMaxBurst) + "), " +
                (epochs ? "epoch (0 ... " + std::to_string(kMaxEpochs - 1) + "), " : std::string()) +
                "target (0 weights, 1 thresholds), module (of those the memory has) or first");
  if (records && cap_records > 0 && first < total) {
    std::vector<PhysFault> v((size_t)std::min<long>(cap_records, total - first));
    hardened_mem_noise_mask(net, hz.scheme, hz.burst, run_seed, layer, target, module, rate_q32, first, v.data(), (long)v.size(), epoch, hz.code,
                            hz.weight_code);
    for (size_t i = 0; i < v.size(); i++) put_record(v[i], records + i * 9);
  }
  return total;
}

long bnn_mi355x_hardened_mem_noise_mask(int scheme, int burst, unsigned long long run_seed, int layer, int target, int module,
                                        unsigned int rate_q32, long first, int *records, int cap_records) {
  return phys_noise_mask("hardened_mem_noise_mask", Hardening{scheme, burst}, run_seed, false, 0, layer, target, module, rate_q32, first, records,
                         cap_records);
}

// the head of the pack_params_* entry points of the physical organisations: the organisation checked, the parameter files read
static bool pack_params_read(const std::string &who, const char *path, int scheme, int code, RawParams &raw) {
  EccOrg eo;
  const std::string le = ecc_layout(rt().spec, scheme, code, 0, eo);
  if (!le.empty()) { fail(who + ": " + le); return false; }
  const std::string e = read_raw_params(rt().spec, path ? path : "", raw);
  if (!e.empty()) { fail(e); return false; }
  return true;
}

// (bnn_mi355x_pack_params_hardened: code 0, and bnn_mi355x_pack_params_ecc) the 9-int fault records applied to the physical
// memories in order, then what the datapath is delivered
static size_t pack_params_phys(const std::string &who, const char *path, int scheme, int code, const int *records, int n_faults, void *dst,
                               size_t cap) {
  const NetSpec &net = rt().spec;
  RawParams raw;
  if (!pack_params_read(who, path, scheme, code, raw)) return 0;
  PhysParams phys;
  phys_load(net, scheme, raw, 0, net.nlayers, phys, code);
  for (int i = 0; i < n_faults; i++)
    if (phys_apply(net, scheme, phys, phys_fault_record(records + i * 9), code) < 0) {
      fail(who + ": fault record out of range (or a module the memory does not have)");
      return 0;
    }
  phys_logical(net, scheme, phys, raw, code);
  return pack_params_out(who, raw, dst, cap);
}

size_t bnn_mi355x_pack_params_hardened(const char *path, int scheme, const int *records, int n_faults, void *dst, size_t cap) {
  return pack_params_phys("pack_params_hardened", path, scheme, EC_NONE, records, n_faults, dst, cap);
}

int *bnn_mi355x_hardened_mem_noise_campaigns(const char *path, int number_class, int scheme, int burst, int num_runs, unsigned long long seed,
                                             const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates, int *image_number,
                                             float *usecPerImage) {
  const MemNoiseEntry en{"hardened_mem_noise_campaigns", &Runtime::hmem_noise_counts, &Runtime::hmem_noise_seeds, true};
  return mem_noise_campaigns_impl(en, Hardening{scheme, burst}, Exposure{0, 0}, path, number_class, num_runs, seed, rate_w_q32, rate_t_q32,
                                  n_rates, image_number, usecPerImage);
}

// ex: scrub_every and repair_every, and the longs of the caller's family (epoch_images is not read: one copy, no images)
static size_t exposure_params_impl(const char *who, const Hardening &hz, const Exposure &ex, unsigned long long run_seed,
                                   const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates, int epoch, void *dst, size_t cap);

// (epoch 0 of a state that is never scrubbed)
size_t bnn_mi355x_hardened_mem_noise_params(int scheme, int burst, unsigned long long run_seed, const unsigned int *rate_w_q32,
                                            const unsigned int *rate_t_q32, int n_rates, void *dst, size_t cap) {
  return exposure_params_impl("hardened_mem_noise_params", Hardening{scheme, burst}, Exposure{1, 0}, run_seed, rate_w_q32, rate_t_q32, n_rates, 0, dst,
                              cap);
}

int bnn_mi355x_last_hardened_mem_noise_counts(long *counts, int cap) { return copy_out(rt().hmem_noise_counts, counts, cap); }

int bnn_mi355x_last_hardened_mem_noise_seeds(unsigned long long *seeds, int cap) { return copy_out(rt().hmem_noise_seeds, seeds, cap); }

// ---- exposure campaigns (the model: mem_org.h) ------------------------------------------------------------------------------

long bnn_mi355x_exposure_mask(int scheme, int burst, unsigned long long run_seed, int epoch, int layer, int target, int module,
                              unsigned int rate_q32, long first, int *records, int cap_records) {
  return phys_noise_mask("exposure_mask", Hardening{scheme, burst}, run_seed, true, epoch, layer, target, module, rate_q32, first, records,
                         cap_records);
}

int *bnn_mi355x_exposure_campaigns(const char *path, int number_class, int scheme, int burst, int num_runs, unsigned long long seed,
                                   const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates, int epoch_images, int scrub_every,
                                   int *image_number, float *usecPerImage) {
  const MemNoiseEntry en{"exposure_campaigns", &Runtime::xmem_counts, &Runtime::xmem_seeds};
  return mem_noise_campaigns_impl(en, Hardening{scheme, burst}, Exposure{epoch_images, scrub_every}, path, number_class, num_runs, seed,
                                  rate_w_q32, rate_t_q32, n_rates, image_number, usecPerImage);
}

// One copy stepped through epochs 0 ... epoch by the campaign's own steps (exposure_begin, exposure_epoch), then read back.
static size_t exposure_params_impl(const char *who, const Hardening &hz, const Exposure &ex, unsigned long long run_seed,
                                   const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates, int epoch, void *dst, size_t cap) {
  Runtime &r = rt();
  if (epoch < 0 || epoch >= kMaxEpochs || ex.scrub_every < 0) {
    fail(std::string(who) + ": epoch must be 0 ... " + std::to_string(kMaxEpochs - 1) + " and scrub_every must not be negative (0: never scrub)");
    return 0;
  }
  if (mem_noise_check(who, rate_w_q32, rate_t_q32, n_rates, hz, false)) return 0;
  if (!dst) return r.blob.size();
  if (cap < r.blob.size()) { fail(std::string(who) + ": destination too small"); return 0; }
  const std::vector<unsigned long long> seeds(1, run_seed);
  const int E = epoch + 1;
  const ExposureCounters cl{1, (size_t)E, (size_t)r.spec.nlayers, ex.longs};  // (the kernels count; nothing reads the counters here)
  MemNoiseJob job;
  auto run = [&]() -> int {
    if (exposure_prepare(who, seeds, rate_w_q32, rate_t_q32, cl, ex, hz, job)) return -1;
    DrainOnFailure drain;  // (declared after the host buffers the queued copies read or write)
    if (settle_handover(r.stream)) return -1;
    if (exposure_begin(seeds, job, 256, cl)) return -1;
    for (int t = 0; t < E; t++)
      if (exposure_epoch(t, rate_w_q32, rate_t_q32, job, 256, cl, ex, hz)) return -1;
    HIP_OK(hipMemcpyAsync(dst, r.d_copies, r.blob.size(), hipMemcpyDeviceToHost, r.stream));
    HIP_OK(hipStreamSynchronize(r.stream));
    drain.ok();
    return 0;
  };
  return run() < 0 ? 0 : r.blob.size();
}

size_t bnn_mi355x_exposure_params(int scheme, int burst, unsigned long long run_seed, const unsigned int *rate_w_q32,
                                  const unsigned int *rate_t_q32, int n_rates, int epoch, int scrub_every, void *dst, size_t cap) {
  return exposure_params_impl("exposure_params", Hardening{scheme, burst}, Exposure{1, scrub_every}, run_seed, rate_w_q32, rate_t_q32, n_rates, epoch,
                              dst, cap);
}

int bnn_mi355x_last_exposure_counts(long *counts, int cap) { return copy_out(rt().xmem_counts, counts, cap); }

int bnn_mi355x_last_exposure_seeds(unsigned long long *seeds, int cap) { return copy_out(rt().xmem_seeds, seeds, cap); }

// ---- coded threshold memories in the exposure campaigns (the code: ecc.h; storage and upsets: mem_org.h) -----------------

unsigned int bnn_mi355x_ecc_encode(unsigned int data) { return ecc_encode(data); }

int bnn_mi355x_ecc_decode(unsigned int data, unsigned int check, unsigned int *out_data) {
  uint32_t d;
  const int status = ecc_decode(data, check, &d);
  if (out_data) *out_data = d;
  return status;
}

int bnn_mi355x_ecc_layout(int scheme, int code, int layer, int out[4]) {
  EccOrg eo;
  const std::string e = ecc_layout(rt().spec, scheme, code, layer, eo);
  if (!e.empty()) return fail("ecc_layout: " + e);
  if (out) { out[0] = eo.org.w_modules; out[1] = eo.org.t_modules; out[2] = eo.org.t_interleave; out[3] = eo.check_bits; }
  return 0;
}

int bnn_mi355x_ecc_check_site(int scheme, int code, int layer, int ind, int bit, int *p_ind, int *p_bit) {
  const NetSpec &net = rt().spec;
  EccOrg eo;
  const std::string e = ecc_layout(net, scheme, code, layer, eo);
  if (!e.empty()) return fail("ecc_check_site: " + e);
  if (!eo.check_bits) return fail("ecc_check_site: layer " + std::to_string(layer) + " has no check memory (code 0, no thresholds, or 24-bit ones)");
  const LayerSpec &L = net.L[layer];
  if (ind < 0 || ind >= L.fold.tmem || bit < 0 || bit >= eo.check_bits) return fail("ecc_check_site: ind or bit outside the check memory");
  int pi, pb;
  interleave_site(eo.org.t_interleave, eo.check_bits, L.fold.tmem, ind, bit, &pi, &pb);
  if (p_ind) *p_ind = pi;
  if (p_bit) *p_bit = pb;
  return 0;
}

long bnn_mi355x_ecc_exposure_mask(int scheme, int code, int burst, unsigned long long run_seed, int epoch, int layer, int target, int module,
                                  unsigned int rate_q32, long first, int *records, int cap_records) {
  return phys_noise_mask("ecc_exposure_mask", Hardening{scheme, burst, code}, run_seed, true, epoch, layer, target, module, rate_q32, first, records,
                         cap_records);
}

size_t bnn_mi355x_pack_params_ecc(const char *path, int scheme, int code, const int *records, int n_faults, void *dst, size_t cap) {
  return pack_params_phys("pack_params_ecc", path, scheme, code, records, n_faults, dst, cap);
}

int *bnn_mi355x_ecc_exposure_campaigns(const char *path, int number_class, int scheme, int code, int burst, int num_runs, unsigned long long seed,
                                       const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates, int epoch_images,
                                       int scrub_every, int *image_number, float *usecPerImage) {
  const MemNoiseEntry en{"ecc_exposure_campaigns", &Runtime::emem_counts, &Runtime::emem_seeds};
  return mem_noise_campaigns_impl(en, Hardening{scheme, burst, code}, Exposure{epoch_images, scrub_every, 6}, path, number_class, num_runs, seed,
                                  rate_w_q32, rate_t_q32, n_rates, image_number, usecPerImage);
}

size_t bnn_mi355x_ecc_exposure_params(int scheme, int code, int burst, unsigned long long run_seed, const unsigned int *rate_w_q32,
                                      const unsigned int *rate_t_q32, int n_rates, int epoch, int scrub_every, void *dst, size_t cap) {
  return exposure_params_impl("ecc_exposure_params", Hardening{scheme, burst, code}, Exposure{1, scrub_every, 6}, run_seed, rate_w_q32, rate_t_q32,
                              n_rates, epoch, dst, cap);
}

int bnn_mi355x_last_ecc_exposure_counts(long *counts, int cap) { return copy_out(rt().emem_counts, counts, cap); }

int bnn_mi355x_last_ecc_exposure_seeds(unsigned long long *seeds, int cap) { return copy_out(rt().emem_seeds, seeds, cap); }

// ---- repair scrubs in the exposure campaigns (the model: mem_org.h, "repair scrubs"; the rule on a code word: ecc.h) -------

int bnn_mi355x_ecc_repair(unsigned int data, unsigned int check, unsigned int *out_data, unsigned int *out_check) {
  uint32_t d, c;
  const int status = ecc_repair(data, check, &d, &c);
  if (out_data) *out_data = d;
  if (out_check) *out_check = c;
  return status;
}

// (bnn_mi355x_pack_params_repair, and with a weight code bnn_mi355x_pack_params_wecc)
static size_t pack_params_replayed(const std::string &who, const char *path, int scheme, int code, int weight_code, const int *records, int n_faults,
                                   void *dst, size_t cap, int weight_interleave = 0) {
  const NetSpec &net = rt().spec;
  RawParams raw;
  if (!pack_params_read(who, path, scheme, code, raw)) return 0;
  PhysParams loaded;
  phys_load(net, scheme, raw, 0, net.nlayers, loaded, code, weight_code, weight_interleave);
  PhysParams phys = loaded;
  const std::string re = phys_replay(net, scheme, code, loaded, phys, records, n_faults, weight_code, weight_interleave);
  if (!re.empty()) { fail(who + ": " + re); return 0; }
  phys_logical(net, scheme, phys, raw, code, nullptr, weight_code, nullptr, weight_interleave);
  return pack_params_out(who, raw, dst, cap);
}

size_t bnn_mi355x_pack_params_repair(const char *path, int scheme, int code, const int *records, int n_faults, void *dst, size_t cap) {
  return pack_params_replayed("pack_params_repair", path, scheme, code, WC_NONE, records, n_faults, dst, cap);
}

int *bnn_mi355x_repair_exposure_campaigns(const char *path, int number_class, int scheme, int code, int burst, int num_runs, unsigned long long seed,
                                          const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates, int epoch_images,
                                          int scrub_every, int repair_every, int *image_number, float *usecPerImage) {
  const MemNoiseEntry en{"repair_exposure_campaigns", &Runtime::rmem_counts, &Runtime::rmem_seeds, false, false, false, true};
  return mem_noise_campaigns_impl(en, Hardening{scheme, burst, code}, Exposure{epoch_images, scrub_every, 8, repair_every}, path, number_class,
                                  num_runs, seed, rate_w_q32, rate_t_q32, n_rates, image_number, usecPerImage);
}

size_t bnn_mi355x_repair_exposure_params(int scheme, int code, int burst, unsigned long long run_seed, const unsigned int *rate_w_q32,
                                         const unsigned int *rate_t_q32, int n_rates, int epoch, int scrub_every, int repair_every, void *dst,
                                         size_t cap) {
  if (repair_every < 0) {
    fail("repair_exposure_params: repair_every must not be negative (0: never repair)");
    return 0;
  }
  return exposure_params_impl("repair_exposure_params", Hardening{scheme, burst, code}, Exposure{1, scrub_every, 8, repair_every}, run_seed, rate_w_q32,
                              rate_t_q32, n_rates, epoch, dst, cap);
}

int bnn_mi355x_last_repair_exposure_counts(long *counts, int cap) { return copy_out(rt().rmem_counts, counts, cap); }

int bnn_mi355x_last_repair_exposure_seeds(unsigned long long *seeds, int cap) { return copy_out(rt().rmem_seeds, seeds, cap); }

// ---- coded weight memories in the exposure campaigns (the code: wecc.h; storage and upsets: mem_org.h) -------------------

unsigned int bnn_mi355x_wecc_encode(unsigned long long data) { return wecc_encode(data); }

int bnn_mi355x_wecc_decode(unsigned long long data, unsigned int check, unsigned long long *out_data) {
  uint64_t d;
  const int status = wecc_decode(data, check, &d);
  if (out_data) *out_data = d;
  return status;
}

int bnn_mi355x_wecc_repair(unsigned long long data, unsigned int check, unsigned long long *out_data, unsigned int *out_check) {
  uint64_t d;
  uint32_t c;
  const int status = wecc_repair(data, check, &d, &c);
  if (out_data) *out_data = d;
  if (out_check) *out_check = c;
  return status;
}

int bnn_mi355x_wecc_layout(int weight_code, int layer, int out[3]) {
  const NetSpec &net = rt().spec;
  const std::string e = wecc_check(weight_code);
  if (!e.empty()) return fail("wecc_layout: " + e);
  if (layer < 0 || layer >= net.nlayers) return fail("wecc_layout: layer must be 0 ... " + std::to_string(net.nlayers - 1));
  const int cwpp = wecc_words_per_pe(net, weight_code, layer);
  if (out) { out[0] = cwpp ? 1 : 0; out[1] = cwpp; out[2] = cwpp ? kWeccCheckBits : 0; }
  return 0;
}

long bnn_mi355x_wecc_exposure_mask(int scheme, int code, int weight_code, int burst, unsigned long long run_seed, int epoch, int layer, int target,
                                   int module, unsigned int rate_q32, long first, int *records, int cap_records) {
  const std::string e = wecc_check(weight_code);
  if (!e.empty()) return fail("wecc_exposure_mask: " + e);
  return phys_noise_mask("wecc_exposure_mask", Hardening{scheme, burst, code, weight_code}, run_seed, true, epoch, layer, target, module, rate_q32,
                         first, records, cap_records);
}

size_t bnn_mi355x_pack_params_wecc(const char *path, int scheme, int code, int weight_code, const int *records, int n_faults, void *dst, size_t cap) {
  const std::string e = wecc_check(weight_code);
  if (!e.empty()) { fail("pack_params_wecc: " + e); return 0; }
  return pack_params_replayed("pack_params_wecc", path, scheme, code, weight_code, records, n_faults, dst, cap);
}

int *bnn_mi355x_wecc_exposure_campaigns(const char *path, int number_class, int scheme, int code, int weight_code, int burst, int num_runs,
                                        unsigned long long seed, const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates,
                                        int epoch_images, int scrub_every, int repair_every, int *image_number, float *usecPerImage) {
  Runtime &r = rt();
  r.wmem_counts.clear();
  r.wmem_seeds.clear();
  const std::string e = wecc_check(weight_code);  // (before a device is looked for, like every refusal of the repair entry point)
  if (!e.empty()) { fail("wecc_exposure_campaigns: " + e); return nullptr; }
  const MemNoiseEntry en{"wecc_exposure_campaigns", &Runtime::wmem_counts, &Runtime::wmem_seeds, false, false, false, true};
  return mem_noise_campaigns_impl(en, Hardening{scheme, burst, code, weight_code}, Exposure{epoch_images, scrub_every, 12, repair_every}, path,
                                  number_class, num_runs, seed, rate_w_q32, rate_t_q32, n_rates, image_number, usecPerImage);
}

size_t bnn_mi355x_wecc_exposure_params(int scheme, int code, int weight_code, int burst, unsigned long long run_seed, const unsigned int *rate_w_q32,
                                       const unsigned int *rate_t_q32, int n_rates, int epoch, int scrub_every, int repair_every, void *dst,
                                       size_t cap) {
  const std::string e = wecc_check(weight_code);
  if (!e.empty()) { fail("wecc_exposure_params: " + e); return 0; }
  if (repair_every < 0) {
    fail("wecc_exposure_params: repair_every must not be negative (0: never repair)");
    return 0;
  }
  return exposure_params_impl("wecc_exposure_params", Hardening{scheme, burst, code, weight_code}, Exposure{1, scrub_every, 12, repair_every}, run_seed,
                              rate_w_q32, rate_t_q32, n_rates, epoch, dst, cap);
}

int bnn_mi355x_last_wecc_exposure_counts(long *counts, int cap) { return copy_out(rt().wmem_counts, counts, cap); }

int bnn_mi355x_last_wecc_exposure_seeds(unsigned long long *seeds, int cap) { return copy_out(rt().wmem_seeds, seeds, cap); }

// ---- column-interleaved code words over the coded weight memories (mem_org.h, "column-interleaved code words") -------------

int bnn_mi355x_iwecc_layout(int weight_code, int weight_interleave, int layer, int out[4]) {
  const NetSpec &net = rt().spec;
  const std::string e = iwecc_check(weight_code, weight_interleave);
  if (!e.empty()) return fail("iwecc_layout: " + e);
  if (layer < 0 || layer >= net.nlayers) return fail("iwecc_layout: layer must be 0 ... " + std::to_string(net.nlayers - 1));
  const int cwpp = wecc_words_per_pe(net, weight_code, layer);
  if (out) {
    out[0] = cwpp ? 1 : 0;
    out[1] = cwpp;
    out[2] = cwpp ? kWeccCheckBits : 0;
    out[3] = wecc_depth(net, weight_code, weight_interleave, layer);
  }
  return 0;
}

int bnn_mi355x_iwecc_site(int weight_code, int weight_interleave, int layer, int module, long index, long out[2]) {
  const NetSpec &net = rt().spec;
  const std::string e = iwecc_check(weight_code, weight_interleave);
  if (!e.empty()) return fail("iwecc_site: " + e);
  if (layer < 0 || layer >= net.nlayers) return fail("iwecc_site: layer must be 0 ... " + std::to_string(net.nlayers - 1));
  if (module != 0 && module != 1) return fail("iwecc_site: module must be 0 (a data site of the weight memory) or 1 (a bit of the check memory)");
  if (!wecc_depth(net, weight_code, weight_interleave, layer))
    return fail("iwecc_site: the weight memory of layer " + std::to_string(layer) + " is not coded (weight_code 0, or CNV layer 0)");
  long word;
  int bit;
  if (!iwecc_site(net, weight_code, weight_interleave, layer, module, index, &word, &bit))
    return fail("iwecc_site: index must be 0 ... " +
                std::to_string((long)net.L[layer].fold.pe * wecc_words_per_pe(net, weight_code, layer) * (module ? kWeccCheckBits : kWeccDataBits) - 1));
  if (out) { out[0] = word; out[1] = bit; }
  return 0;
}

size_t bnn_mi355x_pack_params_iwecc(const char *path, int scheme, int code, int weight_code, int weight_interleave, const int *records, int n_faults,
                                    void *dst, size_t cap) {
  const std::string e = iwecc_check(weight_code, weight_interleave);
  if (!e.empty()) { fail("pack_params_iwecc: " + e); return 0; }
  return pack_params_replayed("pack_params_iwecc", path, scheme, code, weight_code, records, n_faults, dst, cap, weight_interleave);
}

int *bnn_mi355x_iwecc_exposure_campaigns(const char *path, int number_class, int scheme, int code, int weight_code, int weight_interleave, int burst,
                                         int num_runs, unsigned long long seed, const unsigned int *rate_w_q32, const unsigned int *rate_t_q32,
                                         int n_rates, int epoch_images, int scrub_every, int repair_every, int *image_number, float *usecPerImage) {
  Runtime &r = rt();
  r.iwmem_counts.clear();
  r.iwmem_seeds.clear();
  const std::string e = iwecc_check(weight_code, weight_interleave);  // (before a device is looked for, like every refusal of the family)
  if (!e.empty()) { fail("iwecc_exposure_campaigns: " + e); return nullptr; }
  const MemNoiseEntry en{"iwecc_exposure_campaigns", &Runtime::iwmem_counts, &Runtime::iwmem_seeds, false, false, false, true};
  return mem_noise_campaigns_impl(en, Hardening{scheme, burst, code, weight_code, weight_interleave}, Exposure{epoch_images, scrub_every, 12, repair_every},
                                  path, number_class, num_runs, seed, rate_w_q32, rate_t_q32, n_rates, image_number, usecPerImage);
}

size_t bnn_mi355x_iwecc_exposure_params(int scheme, int code, int weight_code, int weight_interleave, int burst, unsigned long long run_seed,
                                        const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates, int epoch, int scrub_every,
                                        int repair_every, void *dst, size_t cap) {
  const std::string e = iwecc_check(weight_code, weight_interleave);
  if (!e.empty()) { fail("iwecc_exposure_params: " + e); return 0; }
  if (repair_every < 0) {
    fail("iwecc_exposure_params: repair_every must not be negative (0: never repair)");
    return 0;
  }
  return exposure_params_impl("iwecc_exposure_params", Hardening{scheme, burst, code, weight_code, weight_interleave},
                              Exposure{1, scrub_every, 12, repair_every}, run_seed, rate_w_q32, rate_t_q32, n_rates, epoch, dst, cap);
}

int bnn_mi355x_last_iwecc_exposure_counts(long *counts, int cap) { return copy_out(rt().iwmem_counts, counts, cap); }

int bnn_mi355x_last_iwecc_exposure_seeds(unsigned long long *seeds, int cap) { return copy_out(rt().iwmem_seeds, seeds, cap); }

void free_results(int *result) { delete[] result; }

void deinit(void) {
  free_workspace();
  rt().warmed = false;  // the buffers the warm-up allocated are gone: the next load warms again
}

const char *bnn_mi355x_network(void) {
#ifdef BNN_VARIANT
  return BNN_VARIANT;
#else
  return rt().spec.name;
#endif
}
int bnn_mi355x_image_bytes(void) { return rt().spec.image_bytes(); }
const char *bnn_mi355x_last_error(void) { return rt().err.c_str(); }

int bnn_mi355x_set_device(int ordinal) {
  Runtime &r = rt();
  if (r.d_blob || r.cap || r.stage_cap || r.stream) {
    if (ordinal == r.device) return 0;  // already bound to exactly this device: nothing to do
    return fail("set_device must be called before load_parameters (this library is bound to device " + std::to_string(r.device) + ")");
  }
  if (ordinal < 0) return fail("set_device: negative ordinal");
  r.device = ordinal;
  return 0;
}

size_t bnn_mi355x_pack_params(const char *path, void *dst, size_t cap) {
  std::vector<uint8_t> blob;
  const std::string e = pack_params_from_dir(rt().spec, path ? path : "", blob);
  if (!e.empty()) { fail(e); return 0; }
  if (dst) {
    if (cap < blob.size()) { fail("pack_params: destination too small"); return 0; }
    std::memcpy(dst, blob.data(), blob.size());
  }
  return blob.size();
}

size_t bnn_mi355x_export_params(void *dst, size_t cap) {
  Runtime &r = rt();
  if (r.blob.empty()) { fail("export_params: nothing loaded"); return 0; }
  if (dst) {
    if (cap < r.blob.size()) { fail("export_params: destination too small"); return 0; }
    std::memcpy(dst, r.blob.data(), r.blob.size());
  }
  return r.blob.size();
}

int bnn_mi355x_import_params(const void *src, size_t bytes) {
  Runtime &r = rt();
  const std::string e = validate_blob(r.spec, src, bytes);
  if (!e.empty()) return fail(e);
  r.blob.assign(static_cast<const uint8_t *>(src), static_cast<const uint8_t *>(src) + bytes);
  r.raw = RawParams{};
  if (upload_blob()) { r.blob.clear(); return -1; }
  r.err.clear();
  (void)warm_up();  // like load_parameters: a failing warm-up is reported (stderr, last_error), the parameters are loaded
  return 0;
}

size_t bnn_mi355x_params_bytes(void) { return blob_bytes(rt().spec); }

int bnn_mi355x_import_params_device(const void *d_src, size_t bytes, void *hip_stream) {
  Runtime &r = rt();
  if (!d_src || bytes != blob_bytes(r.spec)) return fail("import_params_device: size is not this network's blob size");
  if (bind_device()) return -1;
  // The host keeps a copy as well: it validates the header before anything on the device trusts it, and
  // export_params / the fault machinery read it.  ~0.2-0.8 MB once per load.
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  std::vector<uint8_t> host(bytes);
  HIP_OK(hipMemcpyAsync(host.data(), d_src, bytes, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  const std::string e = validate_blob(r.spec, host.data(), bytes);
  if (!e.empty()) return fail(e);
  r.blob.swap(host);
  r.raw = RawParams{};
  if (upload_blob()) { r.blob.clear(); return -1; }
  r.err.clear();
  (void)warm_up();  // (as above)
  return 0;
}

unsigned int bnn_mi355x_params_crc(void) {
  Runtime &r = rt();
  if (r.blob.empty() || !r.d_blob) { fail("params_crc: nothing loaded"); return 0; }
  // of the bytes the GPU actually holds, read back -- not of the host copy
  std::vector<uint8_t> dev(r.d_blob_bytes);
  if (bind_device() || hipStreamSynchronize(r.stream) != hipSuccess ||
      hipMemcpy(dev.data(), r.d_blob, dev.size(), hipMemcpyDeviceToHost) != hipSuccess) {
    fail("params_crc: read-back failed");
    return 0;
  }
  uint32_t crc = 0xFFFFFFFFu;  // CRC-32 (IEEE 802.3, reflected), bitwise: 200 KB once
  for (uint8_t b : dev) {
    crc ^= b;
    for (int k = 0; k < 8; k++) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
  }
  return ~crc;
}

int *bnn_mi355x_inference_buffer(const uint8_t *images, int n_images, int number_class, float *usecPerImage,
                                 int enable_detail) {
  if (!ready()) return nullptr;
  if (n_images < 0 || (n_images > 0 && !images)) { fail("inference_buffer: bad arguments"); return nullptr; }
  return classify_host(images, n_images, number_class, usecPerImage, enable_detail);
}

int bnn_mi355x_binarize_pack(const uint8_t *images, int n_images, uint64_t *words) {
  if (rt().spec.is_cnv) return fail("binarize_pack: the CNV networks take 8-bit inputs (quantised on the GPU)");
  if (n_images < 0 || (n_images > 0 && (!images || !words))) return fail("binarize_pack: bad arguments");
  binarize_pack(images, (size_t)n_images, words);
  return 0;
}

int bnn_mi355x_inference_raw(const uint8_t *images, int n_images, int16_t *scores, uint64_t *words,
                             float *usecPerImage) {
  if (!ready()) return -1;
  if (n_images < 0 || (n_images > 0 && !images)) return fail("inference_raw: bad arguments");
  return infer_host(images, n_images, 64, nullptr, scores, words, usecPerImage);
}

int bnn_mi355x_reserve(int max_images) {
  if (!ready() || reserve(max_images)) return -1;
  // (a CNV pass of kForkMin images and more runs its second half on the second lane: size that workspace now as well, so
  // that the call itself stays free of allocations)
  const int m = max_images < kMaxChunk ? max_images : kMaxChunk;
  if (rt().spec.is_cnv && m >= kForkMin && lanes_for(3) == 2) return reserve2((m + 1) / 2);  // (>= the second half of any pass up to m)
  return 0;
}

#ifdef BNN_LFC_STAMPS
// diagnostic build only: 1024 blocks x 8 wall-clock stamps (100 MHz) of the last k_lfc_block_s launch
int bnn_mi355x_debug_lfc_stamps(unsigned long long *dst) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return bnn::lfc_stamps_read(dst) == hipSuccess ? 0 : -1;
}
// ... and 1024 blocks x 16 waves x 16 stamps
int bnn_mi355x_debug_lfc_wstamps(unsigned long long *dst) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return bnn::lfc_wstamps_read(dst) == hipSuccess ? 0 : -1;
}
#endif

int bnn_mi355x_matrix_stages(int n_images) {
  Runtime &r = rt();
  if (!r.d_blob) return -1;
  if (!r.spec.is_cnv || n_images <= 0) return 0;
  CnvLaunch a{};
  a.n = n_images;
  set_forms(a);
  return cnv_matrix_stages(r.spec.id, a);
}

int bnn_mi355x_chunk_plan(int n_images, int from_file, int *bases, int cap) {
  if (n_images < 0) return fail("chunk_plan: bad arguments");
  const std::vector<int> plan = plan_chunks(n_images, false, from_file != 0);
  for (size_t i = 0; i < plan.size() && (int)i < cap && bases; i++) bases[i] = plan[i];
  return (int)plan.size();
}

long bnn_mi355x_debug_stage_output(const uint8_t *images, int n_images, int stage, void *dst, size_t cap) {
  Runtime &r = rt();
  if (!ready()) return -1;
  int in_buf1 = 0;
  const size_t per = stage_output_bytes(r.spec.is_cnv, r.spec.abits, stage, &in_buf1);
  if (per == 0 || n_images <= 0 || n_images > kHostChunk || !images || !dst || cap < per * (size_t)n_images)
    return fail("debug_stage_output: bad arguments");
  r.debug_last_stage = stage;
  std::vector<uint64_t> w((size_t)n_images);
  const int rc = infer_host(images, n_images, 10, nullptr, nullptr, r.spec.is_cnv ? nullptr : w.data(), nullptr);
  r.debug_last_stage = -1;
  if (rc) return -1;
  HIP_OK(hipMemcpy(dst, in_buf1 ? r.buf1 : r.buf0, per * (size_t)n_images, hipMemcpyDeviceToHost));
  return (long)per;
}

int bnn_mi355x_plan_faults(unsigned long long seed, int num_images, unsigned int flip_count, int word_size, int target,
                           const int *target_layers, unsigned int num_targets, int *records, int cap_records) {
  std::vector<Fault> plan;
  const std::string pe = plan_faults(rt().spec, seed, num_images, flip_count, word_size, target, target_layers, num_targets, plan);
  if (!pe.empty()) return fail(pe);
  for (size_t i = 0; i < plan.size() && (int)i < cap_records; i++) put_record(plan[i], records + i * 8);
  return (int)plan.size();
}

size_t bnn_mi355x_pack_params_faulty(const char *path, const int *records, int n_faults, void *dst, size_t cap) {
  RawParams raw;
  const std::string e = read_raw_params(rt().spec, path ? path : "", raw);
  if (!e.empty()) { fail(e); return 0; }
  for (int i = 0; i < n_faults; i++)
    if (apply_fault(rt().spec, raw, fault_record(records + i * 8)) < 0) { fail("pack_params_faulty: fault record out of range"); return 0; }
  return pack_params_out("pack_params_faulty", raw, dst, cap);
}

int bnn_mi355x_set_fault_seed(unsigned long long seed) {
  rt().fault_seed = seed;
  return 0;
}

int bnn_mi355x_last_faults(int *records, int cap_records) {
  Runtime &r = rt();
  const int n = (int)r.last_faults.size();
  for (int i = 0; i < n && i < cap_records; i++) put_record(r.last_faults[i], records + i * 8);
  return n;
}

int bnn_mi355x_thumbnail_size(int width, int height, int *out_w, int *out_h) {
  int ow = width, oh = height;
  const bool resized = width > 0 && height > 0 && thumbnail_size(width, height, 32, &ow, &oh);
  if (out_w) *out_w = ow;
  if (out_h) *out_h = oh;
  return resized ? 1 : 0;
}

int bnn_mi355x_images_to_cifar(const uint8_t *const *pixels, const int *widths, const int *heights, const int *bands,
                               const long *row_strides, int n_images, uint8_t *records) {
  Runtime &r = rt();
  if (!r.spec.is_cnv) return fail("images_to_cifar: CIFAR-10 records are the input of the CNV networks only");
  if (n_images < 0 || (n_images > 0 && (!pixels || !widths || !heights || !bands || !records)))
    return fail("images_to_cifar: bad arguments");
  if (n_images == 0) return 0;
  if (bind_device()) return -1;
  if (r.d_pp_rec.grow((size_t)n_images * 3073)) return -1;
  // host copies of the coefficient tables must outlive their (asynchronous) upload: kept until the next sync
  std::vector<std::vector<int32_t>> keep;
  // declared after `keep`, so destroyed (= streams drained on a failing exit) before it: uploads from the caller's
  // pictures and from `keep` may still be queued when an error returns
  DrainOnFailure drain;
  int last_w = -1, last_h = -1, ow = 0, oh = 0;
  ResizeTables tabs;
  for (int i = 0; i < n_images; i++) {
    const int w = widths[i], h = heights[i], nb = bands[i];
    if (!pixels[i] || w < 1 || h < 1 || w > 65535 || h > 65535 || (nb != 1 && nb != 3 && nb != 4))
      return fail("images_to_cifar: image " + std::to_string(i) + ": need 1..65535 x 1..65535 pixels of 1 (L), 3 (RGB) or 4 (RGBA) bytes");
    const size_t row_bytes = (size_t)w * nb;
    const long stride = row_strides ? row_strides[i] : (long)row_bytes;
    if (stride < (long)row_bytes) return fail("images_to_cifar: row stride shorter than a row");
    if (w != last_w || h != last_h) {
      ow = w; oh = h;
      (void)thumbnail_size(w, h, 32, &ow, &oh);
      std::vector<int32_t> all;
      tabs = resize_tables(w, h, ow, oh, all);
      if (r.d_pp_coef.grow(all.size())) return -1;
      if (keep.size() >= 16) { HIP_OK(hipStreamSynchronize(r.stream)); keep.clear(); }
      keep.push_back(std::move(all));
      HIP_OK(hipMemcpyAsync(r.d_pp_coef, keep.back().data(), keep.back().size() * sizeof(int32_t), hipMemcpyHostToDevice, r.stream));
      last_w = w; last_h = h;
    }
    if (r.d_pp_src.grow(row_bytes * h) || r.d_pp_tmp.grow((size_t)(h > w ? h : w) * 32 * 4 + 4096)) return -1;
    if (upload_rows(r.d_pp_src, pixels[i], row_bytes, stride, h)) return -1;
    ResampleJob j{};
    j.src = r.d_pp_src; j.w = w; j.h = h; j.bands = nb; j.stride = (long)row_bytes;
    j.out_w = ow; j.out_h = oh;
    j.vertical_first = vertical_pass_first(w, h, oh);
    set_tables(j, r.d_pp_coef, tabs);
    j.tmp = r.d_pp_tmp;
    j.record = r.d_pp_rec + (size_t)i * 3073;
    const hipError_t e = launch_image_to_cifar(j, r.stream);
    if (e != hipSuccess) return launch_failed("images_to_cifar", e);
  }
  HIP_OK(hipMemcpyAsync(records, r.d_pp_rec, (size_t)n_images * 3073, hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  drain.ok();
  return 0;
}

int bnn_mi355x_profile(int enable) {
  Runtime &r = rt();
  r.profiling = enable != 0;
  r.prof_used = 0;
  return 0;
}

int bnn_mi355x_profile_read(float *ms_per_stage, int cap, int *n_chunks) {
  Runtime &r = rt();
  const int stages = r.spec.is_cnv ? kCnvStages : kLfcStages;
  if (!ms_per_stage || cap < stages) return fail("profile_read: need room for all stages");
  for (int i = 0; i < stages; i++) ms_per_stage[i] = 0.f;
  for (size_t k = 0; k < r.prof_used; k++) {
    std::vector<hipEvent_t> &set = r.prof_sets[k];
    HIP_OK(hipEventSynchronize(set[stages]));
    for (int i = 0; i < stages; i++) {
      float ms = 0.f;
      HIP_OK(hipEventElapsedTime(&ms, set[i], set[i + 1]));
      ms_per_stage[i] += ms;
    }
  }
  if (n_chunks) *n_chunks = (int)r.prof_used;
  r.prof_used = 0;
  return stages;
}

const char *bnn_mi355x_stage_name(int stage) { return stage_name(rt().spec.is_cnv, stage); }

int bnn_mi355x_inference_device(const void *d_images, int n_images, int number_class, int32_t *d_classes,
                                int16_t *d_scores, uint64_t *d_words, void *hip_stream) {
  Runtime &r = rt();
  if (!ready()) return -1;
  if (n_images < 0 || (n_images > 0 && !d_images)) return fail("inference_device: bad arguments");
  if (bad_number_class(number_class)) return -1;
  // the kernels read images with 128-bit loads and write scores as dwords (include/bnn_mi355x.h states the alignment)
  auto misaligned = [](const void *p, uintptr_t a) { return p && (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  if (misaligned(d_images, 16)) return fail("inference_device: d_images must be 16-byte aligned");
  if (misaligned(d_classes, 4) || misaligned(d_scores, 4) || misaligned(d_words, 8))
    return fail("inference_device: d_classes / d_scores must be 4-byte aligned, d_words 8-byte aligned");
  // the device-side LFC decode is an exact integer floor(log2); the reference's (unsigned) log2((double) word)
  // rounds UP for some words of 48 bits and more, which only the host decode (libm) reproduces
  if (!r.spec.is_cnv && d_classes && number_class > 47)
    return fail("inference_device: device-side LFC classes need number_class <= 47 (take d_words and decode on the host)");
  if (bind_device()) return -1;  // the calling thread's current device may not be this library's
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const size_t isz = (size_t)r.spec.image_bytes();
  if (!r.spec.is_cnv && !d_words) {  // the LFC decode stage reads the raw words: give it somewhere to put them
    if (reserve_host(1, (size_t)n_images)) return -1;
    d_words = r.d_words;
  }
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &capturing) != hipSuccess) capturing = hipStreamCaptureStatusNone;
  // one pass of at most kMaxChunk images; returns -1 with the error in last_error
  auto pass = [&](int base, int m) -> int {
    const uint8_t *img = static_cast<const uint8_t *>(d_images) + (size_t)base * isz;
    int32_t *cls = d_classes ? d_classes + base : nullptr;
    int16_t *sc = d_scores ? d_scores + (size_t)base * 64 : nullptr;
    uint64_t *wd = d_words ? d_words + base : nullptr;
    // A pass of a CNV net forks over the two compute lanes: first half on the caller's stream, second half on the
    // library's second stream (its own activation workspace), joined before the call returns -- one half's launch gaps
    // and kernel tails are filled by the other's kernels.  tools/two_lane_probe.py (HALVES=2), profiles/
    // r03_device_call_fork_probe.txt: 131 072 images 10.28 -> 10.16 ms, 65 536 5.26 -> 5.13, 32 768 2.69 -> 2.60, 20 000
    // 1.66 -> 1.63; 10 000 images and the LFC nets (one launch per pass) lose, four or eight pieces gain less.  Not while the
    // caller's stream is being captured into a graph, nor with stage profiling on (the stage events would time overlapping
    // kernels), nor under BNN_MI355X_LANES=1.
    const bool fork = r.spec.is_cnv && m >= kForkMin && lanes_for(3) == 2 && capturing == hipStreamCaptureStatusNone;
    if (!fork) return (reserve(m) || enqueue(img, m, number_class, cls, sc, wd, s)) ? -1 : 0;
    const int h = ((m / 2) + 255) & ~255;  // whole blocks of 256 images in the first half
    // (the first workspace is sized for the WHOLE pass although this call uses half of it: the usual "warm-up call, then
    // capture a call of the same size" sequence runs the captured call unforked, and it must not allocate while capturing)
    if (reserve(m) || reserve2(m - h)) return -1;
    if (settle_handover(s)) return -1;  // (before the fork: the second lane inherits the wait through the fork event)
    HIP_OK(hipEventRecord(r.fork_ev, s));
    HIP_OK(hipStreamWaitEvent(r.stream2, r.fork_ev, 0));
    r.ws_seen[1] = r.ws_gen;
    // From here on the second lane is tied to the caller's stream: whatever fails, the join still happens -- work already
    // queued on the library's own stream must not outlive the call unseen (the next call on another stream waits for
    // ws_event, which is recorded on `s` only).
    const bool ok = enqueue(img, h, number_class, cls, sc, wd, s) == 0 &&
                    enqueue(img + (size_t)h * isz, m - h, number_class, cls ? cls + h : nullptr, sc ? sc + (size_t)h * 64 : nullptr,
                            wd ? wd + h : nullptr, r.stream2, nullptr, nullptr, 1) == 0;
    const std::string why = r.err;
    const bool joined = hipEventRecord(r.lane2_done, r.stream2) == hipSuccess && hipStreamWaitEvent(s, r.lane2_done, 0) == hipSuccess;
    if (!joined) (void)hipStreamSynchronize(r.stream2);  // the join itself failed: settle it on the host
    if (!ok) return fail(why);
    return joined ? 0 : fail("inference_device: joining the second compute lane failed");
  };
  int rc = 0;
  for (int base = 0; base < n_images && rc == 0; base += kMaxChunk) rc = pass(base, (n_images - base < kMaxChunk) ? n_images - base : kMaxChunk);
  return n_images > 0 ? hand_over("inference_device", s, capturing, rc) : rc;
}

long bnn_mi355x_tile_boxes(int width, int height, int size, int *boxes, long cap) {
  if (!rt().spec.is_cnv) return fail("tile_boxes: windows become CIFAR-10 records, the input of the CNV networks only");
  const long n = tile_boxes(width, height, size, boxes, cap < 0 ? 0 : cap);
  if (n < 0) return fail("tile_boxes: need a window size of 4 or more (stride = size / 4) and a picture of 1 x 1 pixels or more");
  return n;
}

}  // extern "C"

namespace bnn {
namespace {

static_assert(kWindowMidBytes == BNN_MI355X_WINDOW_LDS_BYTES && kWindowLdsBytes <= 65536, "the header states the window kernel's LDS bound");

// Enqueues, on r.stream: the scene's upload, one upload of boxes + order + tables, the window kernels (one launch per
// size group; the groups of the one-by-one route through launch_image_to_cifar on a packed copy of each window).
// Record i goes to out + i * pitch: 3073-byte records (`label`) or 16-byte aligned 3072-byte bodies.  The caller has
// validated the arguments, bound the device and syncs the stream before `plan` and the caller's pixels go away.
int enqueue_windows(const char *what, const uint8_t *pixels, int width, int height, int bands, long row_stride, const int *boxes, int n,
                    const WindowPlan &plan, std::vector<int32_t> &meta, uint8_t *out, long pitch, int label) {
  Runtime &r = rt();
  const size_t row_bytes = (size_t)width * bands;
  // one buffer: boxes (16-byte aligned, the kernel reads them as int4) | order | tables
  const size_t off_order = (size_t)n * 4, off_coef = off_order + (((size_t)n + 3) & ~(size_t)3);
  meta.assign(off_coef + plan.coef.size(), 0);
  std::memcpy(meta.data(), boxes, (size_t)n * 4 * sizeof(int32_t));
  std::memcpy(meta.data() + off_order, plan.order.data(), (size_t)n * sizeof(int32_t));
  if (!plan.coef.empty()) std::memcpy(meta.data() + off_coef, plan.coef.data(), plan.coef.size() * sizeof(int32_t));
  if (r.d_win_scene.grow(row_bytes * height) || r.d_win_meta.grow(meta.size())) return -1;
  for (const WindowGroup &g : plan.groups)
    if (!g.fused && (r.d_pp_src.grow((size_t)g.w * g.h * bands) || r.d_pp_rec.grow(3073) || r.d_pp_tmp.grow((size_t)(g.h > g.w ? g.h : g.w) * 32 * 4 + 4096)))
      return -1;
  if (upload_rows(r.d_win_scene, pixels, row_bytes, row_stride, height)) return -1;
  HIP_OK(hipMemcpyAsync(r.d_win_meta, meta.data(), meta.size() * sizeof(int32_t), hipMemcpyHostToDevice, r.stream));
  const int32_t *d_coef = r.d_win_meta + off_coef;
  for (const WindowGroup &g : plan.groups) {
    if (g.fused) {
      if (g.horizontal && (size_t)g.h * g.out_w * bands > (size_t)kWindowMidBytes) return fail(std::string(what) + ": internal: a fused group exceeds the LDS budget");
      WindowLaunch a{};
      a.scene = r.d_win_scene; a.stride = (long)row_bytes; a.bands = bands;
      a.boxes = r.d_win_meta; a.order = r.d_win_meta + off_order + g.first;
      a.w = g.w; a.h = g.h; a.out_w = g.out_w; a.out_h = g.out_h;
      a.horizontal = g.horizontal ? 1 : 0; a.vertical = g.vertical ? 1 : 0;
      set_tables(a, d_coef, g);
      a.out = out; a.out_pitch = pitch; a.label = label;
      const hipError_t e = launch_windows_to_cifar(a, g.count, r.stream);
      if (e != hipSuccess) return launch_failed(what, e);
      continue;
    }
    // one by one: a packed device-to-device copy of the window (RGBA: premultiplied in place there, never in the scene),
    // then exactly what images_to_cifar runs for a picture of that size
    for (int k = g.first; k < g.first + g.count; k++) {
      const int i = plan.order[(size_t)k];
      const int *b = boxes + 4 * (size_t)i;
      const size_t wrow = (size_t)g.w * bands;
      HIP_OK(hipMemcpy2DAsync(r.d_pp_src, wrow, r.d_win_scene + (size_t)b[1] * row_bytes + (size_t)b[0] * bands, row_bytes, wrow, (size_t)g.h,
                              hipMemcpyDeviceToDevice, r.stream));
      ResampleJob j{};
      j.src = r.d_pp_src; j.w = g.w; j.h = g.h; j.bands = bands; j.stride = (long)wrow;
      j.out_w = g.out_w; j.out_h = g.out_h;
      j.vertical_first = vertical_pass_first(g.w, g.h, g.out_h);
      set_tables(j, d_coef, g);
      j.tmp = r.d_pp_tmp;
      j.record = label ? out + (size_t)i * pitch : r.d_pp_rec;
      const hipError_t e = launch_image_to_cifar(j, r.stream);
      if (e != hipSuccess) return launch_failed(what, e);
      if (!label) HIP_OK(hipMemcpyAsync(out + (size_t)i * pitch, r.d_pp_rec + 1, 3072, hipMemcpyDeviceToDevice, r.stream));
    }
  }
  return 0;
}

}  // namespace
}  // namespace bnn

extern "C" {

int bnn_mi355x_windows_to_cifar(const uint8_t *pixels, int width, int height, int bands, long row_stride, const int *boxes,
                                int n_windows, uint8_t *records) {
  Runtime &r = rt();
  if (!r.spec.is_cnv) return fail("windows_to_cifar: CIFAR-10 records are the input of the CNV networks only");
  const std::string bad = validate_windows("windows_to_cifar", pixels, width, height, bands, row_stride, boxes, n_windows, records);
  if (!bad.empty()) return fail(bad);
  if (n_windows == 0) return 0;
  if (bind_device()) return -1;
  WindowPlan plan;
  std::vector<int32_t> meta;  // (outlives its asynchronous upload, like `plan`: declared before `drain`)
  plan_windows(boxes, n_windows, bands, plan);
  if (r.d_pp_rec.grow((size_t)n_windows * 3073)) return -1;
  DrainOnFailure drain;
  if (enqueue_windows("windows_to_cifar", pixels, width, height, bands, row_stride, boxes, n_windows, plan, meta, r.d_pp_rec, 3073, 1)) return -1;
  HIP_OK(hipMemcpyAsync(records, r.d_pp_rec, (size_t)n_windows * 3073, hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  drain.ok();
  return 0;
}

int *bnn_mi355x_classify_windows(const uint8_t *pixels, int width, int height, int bands, long row_stride, const int *boxes,
                                 int n_windows, int number_class, float *usecPerImage, float *usecPreprocess, int enable_detail) {
  Runtime &r = rt();
  if (usecPerImage) *usecPerImage = 0.f;
  if (usecPreprocess) *usecPreprocess = 0.f;
  if (!r.spec.is_cnv) { fail("classify_windows: CIFAR-10 records are the input of the CNV networks only"); return nullptr; }
  // (no output buffer of the caller's to check: the result array is the call's own)
  const std::string bad = validate_windows("classify_windows", pixels, width, height, bands, row_stride, boxes, n_windows, pixels);
  if (!bad.empty()) { fail(bad); return nullptr; }
  if (bad_number_class(number_class)) return nullptr;
  const int n = n_windows;
  if (n > 0 && !ready()) return nullptr;
  int *result = new_result((size_t)n * (enable_detail ? number_class : 1));
  if (!result || n == 0) return result;
  // everything that can fail from here on frees `result`
  auto run = [&]() -> int {
    if (bind_device()) return -1;
    WindowPlan plan;
    std::vector<int32_t> meta;
    std::vector<int16_t> scores;
    plan_windows(boxes, n, bands, plan);
    // the pass's workspaces first (they synchronise when they grow), so that nothing is allocated between the kernels
    if (reserve_results((size_t)n) || r.d_win_body.grow((size_t)n * 3072) || ensure_events(r.win_ev, 3)) return -1;
    if (enable_detail) scores.resize((size_t)n * 64);
    DrainOnFailure drain;
    HIP_OK(hipEventRecord(r.win_ev[0], r.stream));
    if (enqueue_windows("classify_windows", pixels, width, height, bands, row_stride, boxes, n, plan, meta, r.d_win_body, 3072, 0)) return -1;
    HIP_OK(hipEventRecord(r.win_ev[1], r.stream));
    // the pass bnn_mi355x_inference_device enqueues, on the same stream, on bodies that never left the device
    if (bnn_mi355x_inference_device(r.d_win_body, n, number_class, enable_detail ? nullptr : r.d_classes, enable_detail ? r.d_scores : nullptr,
                                    nullptr, r.stream))
      return -1;
    HIP_OK(hipEventRecord(r.win_ev[2], r.stream));
    if (enqueue_cnv_results((size_t)n, result, scores)) return -1;
    HIP_OK(hipStreamSynchronize(r.stream));
    drain.ok();
    widen_scores(scores, number_class, result);
    return (usec_per_image(r.win_ev[0], r.win_ev[1], (size_t)n, usecPreprocess) || usec_per_image(r.win_ev[1], r.win_ev[2], (size_t)n, usecPerImage)) ? -1 : 0;
  };
  if (run()) { delete[] result; return nullptr; }
  return result;
}

}  // extern "C"

// ---- the dense scan: every 32 x 32 window of a picture at stride 4 from one pass (cnvW1A1; scan.h) ------------------
namespace bnn {
namespace {

static_assert(kScanMaxSide == BNN_MI355X_SCAN_MAX_SIDE && kScanMaxWindows == BNN_MI355X_SCAN_MAX_WINDOWS &&
                  kScanMaxMapBytes == BNN_MI355X_SCAN_MAX_MAP_BYTES,
              "the header states the scan's limits");

// Empty when this library scans, else the message for last_error
std::string scan_refused(const char *what) {
  const Runtime &r = rt();
  if (!r.spec.is_cnv) return std::string(what) + ": CIFAR-10 records are the input of the CNV networks only";
  if (r.spec.id != NET_CNVW1A1) return std::string(what) + ": the dense scan is built for cnvW1A1 only (this library is " + r.spec.name + ")";
  return "";
}

// the map buffers of one picture (grow-only).  They may be in use by a scan_device call still in flight on a caller's
// stream: growing waits for the whole device, like reserve().
int reserve_scan(const ScanPlan &p) {
  Runtime &r = rt();
  if (p.buf0 <= r.d_scan_buf0.cap && p.buf1 <= r.d_scan_buf1.cap) return 0;
  HIP_OK(hipDeviceSynchronize());
  return (r.d_scan_buf0.grow(p.buf0) || r.d_scan_buf1.grow(p.buf1)) ? -1 : 0;
}

// The tail of a scan, enqueued on s: stages 6..last_stage with the decode on the layer-5 maps of n windows that the scan's
// stages left in r.d_scan_buf0/1 (run_cnv from first_stage 6: their matrix forms included)
hipError_t run_scan_tail(int n, int ncls, int32_t *d_classes, int16_t *d_scores, hipStream_t s, int last_stage) {
  Runtime &r = rt();
  CnvLaunch c{};
  c.n = n; c.buf0 = r.d_scan_buf0; c.buf1 = r.d_scan_buf1;
  for (int l = 0; l < 9; l++) c.rows[l] = r.rows[l];
  set_forms(c);
  c.scores = d_scores; c.classes = d_classes; c.number_class = ncls; c.stream = s;
  c.first_stage = kScanStages; c.last_stage = last_stage;
  return run_cnv(r.spec.id, c);
}

// Enqueues on s: stages 0..min(last_stage, 5) over the picture (run_scan) and, for last_stage >= 6, the existing stages
// 6..8 with the decode on its nx * ny layer-5 pixels (run_cnv from first_stage 6: their matrix forms included).  The
// caller has validated, bound the device and reserved the maps.
int enqueue_scan(const char *what, const uint8_t *d_planes, long row_stride, long plane_stride, const ScanPlan &p, int ncls, int32_t *d_classes,
                 int16_t *d_scores, hipStream_t s, int last_stage = kCnvStages - 1) {
  Runtime &r = rt();
  if (p.buf0 > r.d_scan_buf0.cap || p.buf1 > r.d_scan_buf1.cap) return fail(std::string(what) + ": internal: the picture's maps exceed the scan workspace");
  if (settle_handover(s)) return -1;
  ScanLaunch a{};
  a.planes = d_planes; a.row_stride = row_stride; a.plane_stride = plane_stride; a.plan = p;
  a.buf0 = r.d_scan_buf0; a.buf1 = r.d_scan_buf1;
  for (int l = 0; l < kScanStages; l++) a.rows[l] = r.rows[l];
  a.stream = s;
  a.last_stage = last_stage < kScanStages - 1 ? last_stage : kScanStages - 1;
  hipError_t e = run_scan(a);
  if (e == hipSuccess && last_stage >= kScanStages) e = run_scan_tail(p.nx * p.ny, ncls, d_classes, d_scores, s, last_stage);
  if (e != hipSuccess) return launch_failed(what, e);
  return 0;
}

// Enqueues on r.stream the resize of the scene in r.d_scan_scene (packed rows) to r.d_scan_planes; the tables are in HBM
int enqueue_scan_resize(const char *what, int w, int h, int bands, int out_w, int out_h, const ResizeTables &t) {
  Runtime &r = rt();
  ScanResize j{};
  j.src = r.d_scan_scene; j.w = w; j.h = h; j.bands = bands; j.stride = (long)w * bands;
  j.out_w = out_w; j.out_h = out_h;
  j.vertical_first = vertical_pass_first(w, h, out_h);
  set_tables(j, r.d_scan_coef, t);
  j.tmp = r.d_scan_tmp; j.planes = r.d_scan_planes;
  const hipError_t e = launch_scan_resize(j, r.stream);
  if (e != hipSuccess) return launch_failed(what, e);
  return 0;
}
size_t resize_tmp_bytes(int w, int h, int bands, int out_w, int out_h) {
  const size_t a = (size_t)h * out_w, b = (size_t)out_h * w;
  return (a > b ? a : b) * bands;
}

}  // namespace
}  // namespace bnn

extern "C" {

int bnn_mi355x_scan_grid(int width, int height, int *nx, int *ny) {
  const std::string no = scan_refused("scan_grid");
  if (!no.empty()) return fail(no);
  if (!nx || !ny) return fail("scan_grid: bad arguments (null pointer)");
  ScanPlan p;
  const std::string bad = plan_scan("scan_grid", width, height, p);
  if (!bad.empty()) return fail(bad);
  *nx = p.nx; *ny = p.ny;
  return 0;
}

long bnn_mi355x_scan_boxes(int width, int height, int size, int *boxes, long cap, int *level_w, int *level_h) {
  const std::string no = scan_refused("scan_boxes");
  if (!no.empty()) return fail(no);
  // (plan_scene with a stand-in for the pointers it checks: the same refusals, in the same words, as scan_scene's)
  ScenePlan plan;
  const std::string bad = plan_scene("scan_boxes", &plan, width, height, 3, 0, &size, 1, &plan, plan);
  if (!bad.empty()) return fail(bad);
  if (level_w) *level_w = plan.levels[0].level_w;
  if (level_h) *level_h = plan.levels[0].level_h;
  return scan_boxes(width, height, size, boxes, cap < 0 ? 0 : cap);
}

int *bnn_mi355x_scan_planes(const uint8_t *planes, int width, int height, int number_class, int *nx, int *ny, float *usecPerImage,
                            int enable_detail) {
  Runtime &r = rt();
  if (usecPerImage) *usecPerImage = 0.f;
  const std::string no = scan_refused("scan_planes");
  if (!no.empty()) { fail(no); return nullptr; }
  if (!planes || !nx || !ny) { fail("scan_planes: bad arguments (null pointer)"); return nullptr; }
  ScanPlan p;
  const std::string bad = plan_scan("scan_planes", width, height, p);
  if (!bad.empty()) { fail(bad); return nullptr; }
  if (bad_number_class(number_class)) return nullptr;
  if (!ready()) return nullptr;
  const int n = p.nx * p.ny;
  int *result = new_result((size_t)n * (enable_detail ? number_class : 1));
  if (!result) return nullptr;
  auto run = [&]() -> int {
    if (bind_device()) return -1;
    std::vector<int16_t> scores;
    const size_t plane = (size_t)width * height;
    if (reserve_results((size_t)n) || r.d_scan_planes.grow(3 * plane) || reserve_scan(p) || ensure_events(r.scan_ev, 2)) return -1;
    if (enable_detail) scores.resize((size_t)n * 64);
    DrainOnFailure drain;
    HIP_OK(hipMemcpyAsync(r.d_scan_planes, planes, 3 * plane, hipMemcpyHostToDevice, r.stream));
    HIP_OK(hipEventRecord(r.scan_ev[0], r.stream));
    if (enqueue_scan("scan_planes", r.d_scan_planes, width, (long)plane, p, number_class, enable_detail ? nullptr : r.d_classes,
                     enable_detail ? r.d_scores : nullptr, r.stream))
      return -1;
    HIP_OK(hipEventRecord(r.scan_ev[1], r.stream));
    if (enqueue_cnv_results((size_t)n, result, scores)) return -1;
    HIP_OK(hipStreamSynchronize(r.stream));
    drain.ok();
    widen_scores(scores, number_class, result);
    return usec_per_image(r.scan_ev[0], r.scan_ev[1], (size_t)n, usecPerImage);
  };
  if (run()) { delete[] result; return nullptr; }
  *nx = p.nx; *ny = p.ny;
  return result;
}

int bnn_mi355x_scan_device(const void *d_planes, int width, int height, int number_class, int32_t *d_classes, int16_t *d_scores,
                           void *hip_stream) {
  const std::string no = scan_refused("scan_device");
  if (!no.empty()) return fail(no);
  if (!d_planes) return fail("scan_device: bad arguments (null pointer)");
  ScanPlan p;
  const std::string bad = plan_scan("scan_device", width, height, p);
  if (!bad.empty()) return fail(bad);
  if (bad_number_class(number_class)) return -1;
  auto misaligned = [](const void *q, uintptr_t a) { return q && (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; };
  if (misaligned(d_classes, 4) || misaligned(d_scores, 4)) return fail("scan_device: d_classes / d_scores must be 4-byte aligned");
  if (!ready()) return -1;
  if (bind_device() || reserve_scan(p)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &capturing) != hipSuccess) capturing = hipStreamCaptureStatusNone;
  const int rc = enqueue_scan("scan_device", static_cast<const uint8_t *>(d_planes), width, (long)width * height, p, number_class, d_classes, d_scores, s);
  return hand_over("scan_device", s, capturing, rc);
}

int *bnn_mi355x_scan_scene(const uint8_t *pixels, int width, int height, int bands, long row_stride, const int *sizes, int n_sizes,
                           int number_class, int *boxes_out, float *usecPerImage, float *usecPreprocess, int enable_detail) {
  Runtime &r = rt();
  if (usecPerImage) *usecPerImage = 0.f;
  if (usecPreprocess) *usecPreprocess = 0.f;
  const std::string no = scan_refused("scan_scene");
  if (!no.empty()) { fail(no); return nullptr; }
  ScenePlan plan;
  const std::string bad = plan_scene("scan_scene", pixels, width, height, bands, row_stride, sizes, n_sizes, boxes_out, plan);
  if (!bad.empty()) { fail(bad); return nullptr; }
  if (bad_number_class(number_class)) return nullptr;
  if (!ready()) return nullptr;
  const size_t n = (size_t)plan.windows;
  int *result = new_result(n * (enable_detail ? number_class : 1));
  if (!result) return nullptr;
  auto run = [&]() -> int {
    if (bind_device()) return -1;
    std::vector<int16_t> scores;
    std::vector<int32_t> coef;  // (outlives its asynchronous upload: declared before `drain`)
    std::vector<ResizeTables> tabs(plan.levels.size());
    size_t planes_need = 0, tmp_need = 1;
    ScanPlan largest;
    for (size_t k = 0; k < plan.levels.size(); k++) {
      const ScanLevel &lv = plan.levels[k];
      if (lv.resized) {
        tabs[k] = resize_tables(width, height, lv.level_w, lv.level_h, coef);
        tmp_need = std::max(tmp_need, resize_tmp_bytes(width, height, bands, lv.level_w, lv.level_h));
      }
      planes_need = std::max(planes_need, (size_t)3 * lv.level_w * lv.level_h);
      largest.buf0 = std::max(largest.buf0, lv.plan.buf0);
      largest.buf1 = std::max(largest.buf1, lv.plan.buf1);
    }
    // every workspace first (they synchronise when they grow), so that nothing is allocated between the kernels
    if (reserve_results(n) || r.d_scan_scene.grow((size_t)width * height * bands) || r.d_scan_planes.grow(planes_need) ||
        r.d_scan_tmp.grow(tmp_need) || r.d_scan_coef.grow(coef.size() + 1) || reserve_scan(largest) ||
        ensure_events(r.scan_ev, 2 * plan.levels.size() + 1))
      return -1;
    if (enable_detail) scores.resize(n * 64);
    DrainOnFailure drain;
    HIP_OK(hipEventRecord(r.scan_ev[0], r.stream));
    if (upload_rows(r.d_scan_scene, pixels, (size_t)width * bands, row_stride, height)) return -1;
    if (!coef.empty()) HIP_OK(hipMemcpyAsync(r.d_scan_coef, coef.data(), coef.size() * sizeof(int32_t), hipMemcpyHostToDevice, r.stream));
    for (size_t k = 0; k < plan.levels.size(); k++) {
      const ScanLevel &lv = plan.levels[k];
      // (a level of the picture's own size: Image.resize returns a copy -- the same kernels only re-lay it out)
      if (enqueue_scan_resize("scan_scene", width, height, bands, lv.level_w, lv.level_h, tabs[k])) return -1;
      HIP_OK(hipEventRecord(r.scan_ev[2 * k + 1], r.stream));
      if (enqueue_scan("scan_scene", r.d_scan_planes, lv.level_w, (long)lv.level_w * lv.level_h, lv.plan, number_class,
                       enable_detail ? nullptr : r.d_classes + lv.first, enable_detail ? r.d_scores + (size_t)lv.first * 64 : nullptr, r.stream))
        return -1;
      HIP_OK(hipEventRecord(r.scan_ev[2 * k + 2], r.stream));
    }
    if (enqueue_cnv_results(n, result, scores)) return -1;
    HIP_OK(hipStreamSynchronize(r.stream));
    drain.ok();
    widen_scores(scores, number_class, result);
    float pre = 0.f, pass = 0.f;
    for (size_t k = 0; k < plan.levels.size(); k++) {
      float a = 0.f, b = 0.f;
      HIP_OK(hipEventElapsedTime(&a, r.scan_ev[2 * k], r.scan_ev[2 * k + 1]));
      HIP_OK(hipEventElapsedTime(&b, r.scan_ev[2 * k + 1], r.scan_ev[2 * k + 2]));
      pre += a; pass += b;
    }
    if (usecPreprocess) *usecPreprocess = pre * 1000.f / (float)n;
    if (usecPerImage) *usecPerImage = pass * 1000.f / (float)n;
    return 0;
  };
  if (run()) { delete[] result; return nullptr; }
  for (const ScanLevel &lv : plan.levels) scan_boxes(width, height, lv.size, boxes_out + 4 * (size_t)lv.first, (long)lv.plan.nx * lv.plan.ny);
  return result;
}

long bnn_mi355x_debug_scan_stage(const uint8_t *planes, int width, int height, int stage, void *out, size_t cap, int *map_w, int *map_h) {
  Runtime &r = rt();
  const std::string no = scan_refused("debug_scan_stage");
  if (!no.empty()) return fail(no);
  if (!planes || !out || !map_w || !map_h || stage < 0 || stage >= kScanStages) return fail("debug_scan_stage: bad arguments");
  ScanPlan p;
  const std::string bad = plan_scan("debug_scan_stage", width, height, p);
  if (!bad.empty()) return fail(bad);
  const size_t bytes = scan_stage_bytes(p, stage);
  if (cap < bytes) return fail("debug_scan_stage: the stage's map takes " + std::to_string(bytes) + " bytes");
  if (!ready() || bind_device()) return -1;
  const size_t plane = (size_t)width * height;
  if (r.d_scan_planes.grow(3 * plane) || reserve_scan(p)) return -1;
  DrainOnFailure drain;
  HIP_OK(hipMemcpyAsync(r.d_scan_planes, planes, 3 * plane, hipMemcpyHostToDevice, r.stream));
  if (enqueue_scan("debug_scan_stage", r.d_scan_planes, width, (long)plane, p, 1, nullptr, nullptr, r.stream, stage)) return -1;
  HIP_OK(hipMemcpyAsync(out, (stage & 1) ? r.d_scan_buf1 : r.d_scan_buf0, bytes, hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  drain.ok();
  *map_w = p.w[stage]; *map_h = p.h[stage];
  return (long)bytes;
}

int bnn_mi355x_scan_resize(const uint8_t *pixels, int width, int height, int bands, long row_stride, int out_w, int out_h,
                           uint8_t *planes) {
  Runtime &r = rt();
  const std::string no = scan_refused("scan_resize");
  if (!no.empty()) return fail(no);
  if (!pixels || !planes) return fail("scan_resize: bad arguments (null pointer)");
  if (bands != 1 && bands != 3) return fail("scan_resize: bands must be 1 (L) or 3 (RGB) bytes per pixel");
  if (width < 1 || height < 1 || out_w < 1 || out_h < 1 || width > kScanMaxSide || height > kScanMaxSide || out_w > kScanMaxSide || out_h > kScanMaxSide)
    return fail("scan_resize: need a picture and a level of 1.." + std::to_string(kScanMaxSide) + " pixels a side");
  if (row_stride != 0 && row_stride < (long)width * bands) return fail("scan_resize: row stride shorter than a row");
  if (bind_device()) return -1;
  std::vector<int32_t> coef;
  const ResizeTables t = resize_tables(width, height, out_w, out_h, coef);
  const size_t out_bytes = (size_t)3 * out_w * out_h;
  if (r.d_scan_scene.grow((size_t)width * height * bands) || r.d_scan_planes.grow(out_bytes) ||
      r.d_scan_tmp.grow(resize_tmp_bytes(width, height, bands, out_w, out_h)) || r.d_scan_coef.grow(coef.size() + 1))
    return -1;
  DrainOnFailure drain;
  if (upload_rows(r.d_scan_scene, pixels, (size_t)width * bands, row_stride, height)) return -1;
  HIP_OK(hipMemcpyAsync(r.d_scan_coef, coef.data(), coef.size() * sizeof(int32_t), hipMemcpyHostToDevice, r.stream));
  if (enqueue_scan_resize("scan_resize", width, height, bands, out_w, out_h, t)) return -1;
  HIP_OK(hipMemcpyAsync(planes, r.d_scan_planes, out_bytes, hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  drain.ok();
  return 0;
}

}  // extern "C"

// ---- the clip scan: all frames and levels of a clip through one launch per stage (cnvW1A1; scan_clip.h) ---------------
namespace bnn {
namespace {

static_assert(kScanClipMaxFrames == BNN_MI355X_SCAN_CLIP_MAX_FRAMES && kScanClipMaxBytes == BNN_MI355X_SCAN_CLIP_MAX_BYTES,
              "the header states the clip scan's limits");

// what one clip call keeps alive until its stream is idle (declared before the call's DrainOnFailure)
struct ClipJob {
  ClipTables tables;
  std::vector<int32_t> coef;
  std::vector<ResizeTables> tabs;
  size_t tmp_frame = 1;  // bytes of one frame's first resize pass, the largest of the levels
};

// Where a clip call's frames come from (include/bnn_mi355x.h, "Camera frames").  Not raw: the plan's bands and strides
// describe RGB or L frames, as the older entry points take them.  Raw: `frames` and `layout` do, and k_unpack_frames
// makes the RGB frames at r.d_scan_scene.  A device source is read where it lies and the call runs on the caller's stream.
struct ClipSource {
  const uint8_t *pixels = nullptr;
  bool device = false, raw = false;
  Frames frames{};
  PixLayout layout{};
  hipStream_t stream = nullptr;  // r.stream for a host source
  size_t raw_bytes() const { return raw && !device ? layout.frame_span * (size_t)layout.n_frames : 0; }
};

// every workspace of a clip call (grow-only; the map buffers are the scan's and grow as they do, behind a device
// synchronise), and the level's Lanczos tables, built once for all frames; raw_bytes: of uploaded raw frames (0: none)
int reserve_clip(const ClipPlan &p, ClipJob &job, size_t raw_bytes = 0) {
  if (raw_bytes && rt().d_clip_raw.grow(raw_bytes)) return -1;
  Runtime &r = rt();
  clip_tables(p, job.tables);
  job.tabs.assign(p.scene.levels.size(), ResizeTables{});
  for (size_t k = 0; k < p.scene.levels.size(); k++) {
    const ScanLevel &lv = p.scene.levels[k];
    if (!lv.resized) continue;
    job.tabs[k] = resize_tables(p.width, p.height, lv.level_w, lv.level_h, job.coef);
    job.tmp_frame = std::max(job.tmp_frame, resize_tmp_bytes(p.width, p.height, p.bands, lv.level_w, lv.level_h));
  }
  ScanPlan maps;
  maps.buf0 = p.buf0; maps.buf1 = p.buf1;
  return (r.d_scan_scene.grow((size_t)p.width * p.height * p.bands * p.frames) || r.d_scan_planes.grow(p.planes_bytes) ||
          r.d_scan_tmp.grow(job.tmp_frame * p.frames) || r.d_scan_coef.grow(job.coef.size() + 1) ||
          r.d_scan_clip_tab.grow(job.tables.words.size()) || reserve_scan(maps))
             ? -1 : 0;
}

// Enqueues on s the copy of `frames` frames of `rows` rows of row_bytes, rows_apart and frames_apart bytes apart at src, to
// packed frames of packed rows at dst: one copy when the frames (or all rows) lie evenly apart, else one 2-D copy a frame
int copy_spaced(uint8_t *dst, const uint8_t *src, size_t row_bytes, size_t rows, size_t rows_apart, size_t frames_apart, int frames, hipMemcpyKind kind,
                hipStream_t s) {
  const size_t frame_bytes = row_bytes * rows;
  if (rows_apart == row_bytes) {  // packed rows: a frame is one run of bytes
    if (frames_apart == frame_bytes) HIP_OK(hipMemcpyAsync(dst, src, frame_bytes * frames, kind, s));
    else HIP_OK(hipMemcpy2DAsync(dst, frame_bytes, src, frames_apart, frame_bytes, (size_t)frames, kind, s));
    return 0;
  }
  if (frames_apart == rows_apart * rows) {  // the rows of all frames lie one stride apart
    HIP_OK(hipMemcpy2DAsync(dst, row_bytes, src, rows_apart, row_bytes, rows * (size_t)frames, kind, s));
    return 0;
  }
  for (int f = 0; f < frames; f++)
    HIP_OK(hipMemcpy2DAsync(dst + (size_t)f * frame_bytes, row_bytes, src + (size_t)f * frames_apart, rows_apart, row_bytes, rows, kind, s));
  return 0;
}

// Enqueues on s the copy of the clip to packed frames at r.d_scan_scene (copy_spaced; the upload of a host clip by default)
int upload_clip(const ClipPlan &p, const uint8_t *pixels, hipMemcpyKind kind = hipMemcpyHostToDevice, hipStream_t s = rt().stream) {
  const size_t row_bytes = (size_t)p.width * p.bands;
  const size_t rows_apart = p.row_stride ? (size_t)p.row_stride : row_bytes, frames_apart = p.frame_stride ? (size_t)p.frame_stride : rows_apart * p.height;
  return copy_spaced(rt().d_scan_scene, pixels, row_bytes, (size_t)p.height, rows_apart, frames_apart, p.frames, kind, s);
}

// Enqueues on s the upload of host raw frames to dst.  The planes of a frame keep their row stride (a frame is ONE run of
// frame_span bytes whatever its format; the kernel reads the width columns only) and the frames follow one another: one
// copy, flat when the frames lie evenly apart and 2-D otherwise.  uploaded_layout states where they then lie.
int upload_raw(uint8_t *dst, const uint8_t *pixels, const PixLayout &l, hipStream_t s) {
  return copy_spaced(dst, pixels, l.frame_span, 1, l.frame_span, l.frames_apart, l.n_frames, hipMemcpyHostToDevice, s);
}
PixLayout uploaded_layout(const PixLayout &l) {
  PixLayout p = l;
  p.frames_apart = l.frame_span;
  return p;
}

// Enqueues on the source's stream: the frames' way to packed RGB or L frames in HBM, the upload of the tables, the resizes of
// every level (one pair of launches a level for all frames), then stages 0..min(last_stage, 5) over all maps (run_scan_clip)
// and, for last_stage >= 6, stages 6..8 with the decode ONCE on all windows.  mid (may be null) is recorded between the
// resizes and the stages.  The caller has validated, bound the device and reserved (reserve_clip, reserve_results).
//   host RGB / L    the upload of the clip (upload_clip)
//   host raw        the upload of the raw planes, then k_unpack_frames
//   device raw      k_unpack_frames reads the caller's memory
//   device RGB / L  packed frames are resized where they lie, others take one device-to-device copy
int enqueue_clip(const char *what, const ClipPlan &p, const ClipJob &job, const ClipSource &src, int ncls, int32_t *d_classes, int16_t *d_scores,
                 hipEvent_t mid, int last_stage) {
  Runtime &r = rt();
  const hipStream_t s = src.stream;
  const size_t frame_bytes = (size_t)p.width * p.height * p.bands;
  const bool in_place = src.device && !src.raw && (p.row_stride == 0 || (size_t)p.row_stride == (size_t)p.width * p.bands) &&
                        (p.frame_stride == 0 || (size_t)p.frame_stride == frame_bytes);
  if (p.buf0 > r.d_scan_buf0.cap || p.buf1 > r.d_scan_buf1.cap || p.planes_bytes > r.d_scan_planes.cap || job.tables.words.size() > r.d_scan_clip_tab.cap ||
      job.tmp_frame * p.frames > r.d_scan_tmp.cap || (!in_place && frame_bytes * p.frames > r.d_scan_scene.cap) || src.raw_bytes() > r.d_clip_raw.cap)
    return fail(std::string(what) + ": internal: the clip exceeds the scan workspace");
  if (settle_handover(s)) return -1;
  const uint8_t *scene = in_place ? src.pixels : r.d_scan_scene.get();
  if (src.raw) {
    UnpackLaunch u{};
    u.src = src.pixels; u.dst = r.d_scan_scene; u.frames = src.frames; u.layout = src.layout; u.stream = s;
    if (!src.device) {
      if (upload_raw(r.d_clip_raw, src.pixels, src.layout, s)) return -1;
      u.src = r.d_clip_raw; u.layout = uploaded_layout(src.layout);
    }
    const hipError_t e = run_unpack_frames(u);
    if (e != hipSuccess) return launch_failed(what, e);
  } else if (!in_place) {
    if (upload_clip(p, src.pixels, src.device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s)) return -1;
  }
  if (!job.coef.empty()) HIP_OK(hipMemcpyAsync(r.d_scan_coef, job.coef.data(), job.coef.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(r.d_scan_clip_tab, job.tables.words.data(), job.tables.words.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  for (size_t k = 0; k < p.scene.levels.size(); k++) {
    const ScanLevel &lv = p.scene.levels[k];
    // (a level of the frames' own size: the same kernels only re-lay it out, as in scan_scene)
    ScanClipResize j{};
    j.src = scene; j.frames = p.frames; j.w = p.width; j.h = p.height; j.bands = p.bands;
    j.stride = (long)p.width * p.bands; j.src_frame = (long)frame_bytes;
    j.out_w = lv.level_w; j.out_h = lv.level_h;
    j.vertical_first = vertical_pass_first(p.width, p.height, lv.level_h);
    set_tables(j, r.d_scan_coef, job.tabs[k]);
    j.tmp = r.d_scan_tmp; j.tmp_frame = (long)job.tmp_frame;
    j.planes = r.d_scan_planes + p.level_planes[k];
    const hipError_t e = launch_clip_resize(j, s);
    if (e != hipSuccess) return launch_failed(what, e);
  }
  if (mid) HIP_OK(hipEventRecord(mid, s));
  ScanClipLaunch a{};
  a.planes = r.d_scan_planes; a.buf0 = r.d_scan_buf0; a.buf1 = r.d_scan_buf1;
  for (int l = 0; l < kScanStages; l++) {
    a.rows[l] = r.rows[l];
    a.desc[l] = job.tables.desc[l]; a.block_map[l] = job.tables.block_map[l]; a.blocks[l] = p.blocks[l];
  }
  a.tables = r.d_scan_clip_tab;
  a.stream = s;
  a.last_stage = last_stage < kScanStages - 1 ? last_stage : kScanStages - 1;
  hipError_t e = run_scan_clip(a);
  if (e == hipSuccess && last_stage >= kScanStages) e = run_scan_tail((int)p.windows, ncls, d_classes, d_scores, s, last_stage);
  if (e != hipSuccess) return launch_failed(what, e);
  return 0;
}

static_assert(sizeof(Frames) == sizeof(bnn_mi355x_frames) && offsetof(Frames, frame_stride) == offsetof(bnn_mi355x_frames, frame_stride),
              "Frames is bnn_mi355x_frames");
static_assert(kPixMaxSide == BNN_MI355X_SCAN_MAX_SIDE && kPixMaxFrames == BNN_MI355X_SCAN_CLIP_MAX_FRAMES && kPixMaxBytes == BNN_MI355X_SCAN_CLIP_MAX_BYTES,
              "the frames' limits are the clip scan's");

// What a clip entry point was asked for.  The *_frames and *_device ones hand `frames` over (null is refused); the older
// ones (n_frames .. row_stride), whose bands state RGB or L.
struct ClipRequest {
  const char *what;
  const void *pixels;
  bool by_frames;
  const Frames *frames;
  int n_frames;
  long frame_stride;
  int width, height, bands;
  long row_stride;
  bool device;
  void *hip_stream;
};
ClipRequest frames_request(const char *what, const void *pixels, const bnn_mi355x_frames *frames, bool device, void *hip_stream) {
  return ClipRequest{what, pixels, true, reinterpret_cast<const Frames *>(frames), 0, 0, 0, 0, 0, 0, device, hip_stream};
}

// plan_clip for a request: empty, or the message for last_error.  Raw frames are validated by validate_frames, and the plan
// is that of the packed RGB frames k_unpack_frames makes of them; RGB and L frames are planned as the older entry points' are.
std::string plan_request(const ClipRequest &q, const int *sizes, int n_sizes, const void *out, ClipPlan &plan, ClipSource &src) {
  src = ClipSource{};
  src.pixels = static_cast<const uint8_t *>(q.pixels);
  src.device = q.device;
  if (!q.by_frames) return plan_clip(q.what, q.pixels, q.n_frames, q.frame_stride, q.width, q.height, q.bands, q.row_stride, sizes, n_sizes, out, plan);
  const std::string bad = validate_frames(q.what, q.frames, q.pixels, src.layout);
  if (!bad.empty()) return bad;
  const Frames &f = *q.frames;
  src.frames = f;
  src.raw = f.format != PIX_RGB && f.format != PIX_L;
  return plan_clip(q.what, q.pixels, f.n_frames, src.raw ? 0 : f.frame_stride, f.width, f.height, f.format == PIX_L ? 1 : 3, src.raw ? 0 : f.row_stride,
                   sizes, n_sizes, out, plan);
}

// A device clip call waits for its stream and hands its results to the host: empty, or the refusal while that stream is
// being captured (nothing has been enqueued or allocated: the capture stays valid)
std::string capture_refused(const ClipRequest &q) {
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (!q.device || hipStreamIsCapturing(static_cast<hipStream_t>(q.hip_stream), &capturing) != hipSuccess || capturing == hipStreamCaptureStatusNone)
    return "";
  return std::string(q.what) + ": hip_stream is being captured: the call waits for its stream and returns its results on the host, which a graph cannot record";
}

// On a failing exit of a device clip call nothing may still be queued on the caller's stream that reads the call's host
// buffers (DrainOnFailure waits for the library's own streams)
struct DrainCaller {
  const ClipSource &src;
  bool armed = true;
  void ok() { armed = false; }
  ~DrainCaller() {
    if (armed && src.device) (void)hipStreamSynchronize(src.stream);
  }
};

// bnn_mi355x_scan_clip, _scan_clip_frames and _scan_clip_device.  A device call settles the workspaces' hand-over before
// it enqueues (enqueue_clip) and has waited for its stream when it returns: it leaves nothing to hand over.
int *scan_clip_call(const ClipRequest &q, const int *sizes, int n_sizes, int number_class, int *boxes_out, float *usecPerImage, float *usecPreprocess,
                    int enable_detail) {
  Runtime &r = rt();
  if (usecPerImage) *usecPerImage = 0.f;
  if (usecPreprocess) *usecPreprocess = 0.f;
  const std::string no = scan_refused(q.what);
  if (!no.empty()) { fail(no); return nullptr; }
  ClipPlan plan;
  ClipSource src;
  const std::string bad = plan_request(q, sizes, n_sizes, boxes_out, plan, src);
  if (!bad.empty()) { fail(bad); return nullptr; }
  if (bad_number_class(number_class)) return nullptr;
  if (!ready()) return nullptr;
  const std::string captured = capture_refused(q);
  if (!captured.empty()) { fail(captured); return nullptr; }
  const size_t n = (size_t)plan.windows;
  int *result = new_result(n * (enable_detail ? number_class : 1));
  if (!result) return nullptr;
  auto run = [&]() -> int {
    if (bind_device()) return -1;
    const hipStream_t s = src.stream = q.device ? static_cast<hipStream_t>(q.hip_stream) : r.stream;
    std::vector<int16_t> scores;
    ClipJob job;  // (outlives its asynchronous uploads: declared before `drain`)
    // every workspace first (they synchronise when they grow), so that nothing is allocated between the kernels
    if (reserve_results(n) || reserve_clip(plan, job, src.raw_bytes()) || ensure_events(r.scan_ev, 3)) return -1;
    if (enable_detail) scores.resize(n * 64);
    DrainOnFailure drain;
    DrainCaller caller{src};
    HIP_OK(hipEventRecord(r.scan_ev[0], s));
    if (enqueue_clip(q.what, plan, job, src, number_class, enable_detail ? nullptr : r.d_classes, enable_detail ? r.d_scores : nullptr, r.scan_ev[1],
                     kCnvStages - 1))
      return -1;
    HIP_OK(hipEventRecord(r.scan_ev[2], s));
    if (enqueue_cnv_results(n, result, scores, s)) return -1;
    HIP_OK(hipStreamSynchronize(s));
    drain.ok();
    caller.ok();
    widen_scores(scores, number_class, result);
    return (usec_per_image(r.scan_ev[0], r.scan_ev[1], n, usecPreprocess) || usec_per_image(r.scan_ev[1], r.scan_ev[2], n, usecPerImage)) ? -1 : 0;
  };
  if (run()) { delete[] result; return nullptr; }
  // (the boxes are the same for every frame: one frame's, exactly what scan_scene writes)
  for (const ScanLevel &lv : plan.scene.levels)
    scan_boxes(plan.width, plan.height, lv.size, boxes_out + 4 * (size_t)lv.first, (long)lv.plan.nx * lv.plan.ny);
  return result;
}

}  // namespace
}  // namespace bnn

extern "C" {

int bnn_mi355x_scan_clip_capacity(int width, int height, const int *sizes, int n_sizes) {
  const std::string no = scan_refused("scan_clip_capacity");
  if (!no.empty()) return fail(no);
  std::string why;
  const int cap = scan_clip_capacity("scan_clip_capacity", width, height, sizes, n_sizes, why);
  if (cap < 1) { fail(why); return 0; }
  return cap;
}

int bnn_mi355x_scan_clip_layout(int width, int height, const int *sizes, int n_sizes, int n_frames, int *map_w, int *map_h, long *offsets,
                                long *first, int *level_size, long *buf_bytes) {
  const std::string no = scan_refused("scan_clip_layout");
  if (!no.empty()) return fail(no);
  // (plan_clip with a stand-in for the pointers it checks: RGB frames, packed)
  ClipPlan p;
  const std::string bad = plan_clip("scan_clip_layout", sizes ? (const void *)&p : nullptr, n_frames, 0, width, height, 3, 0, sizes, n_sizes, &p, p);
  if (!bad.empty()) return fail(bad);
  for (size_t m = 0; m < p.maps.size(); m++) {
    const ClipMap &cm = p.maps[m];
    const ScanLevel &lv = p.scene.levels[(size_t)cm.level];
    for (int s = 0; s < kScanStages; s++) {
      if (map_w) map_w[m * kScanStages + s] = lv.plan.w[s];
      if (map_h) map_h[m * kScanStages + s] = lv.plan.h[s];
      if (offsets) offsets[m * kScanStages + s] = (long)cm.off[s];
    }
    if (first) first[m] = cm.first;
    if (level_size) level_size[m] = lv.size;
  }
  if (buf_bytes) { buf_bytes[0] = (long)p.buf0; buf_bytes[1] = (long)p.buf1; }
  return (int)p.maps.size();
}

int *bnn_mi355x_scan_clip(const uint8_t *pixels, int n_frames, long frame_stride, int width, int height, int bands, long row_stride,
                          const int *sizes, int n_sizes, int number_class, int *boxes_out, float *usecPerImage, float *usecPreprocess,
                          int enable_detail) {
  const ClipRequest q{"scan_clip", pixels, false, nullptr, n_frames, frame_stride, width, height, bands, row_stride, false, nullptr};
  return scan_clip_call(q, sizes, n_sizes, number_class, boxes_out, usecPerImage, usecPreprocess, enable_detail);
}

int *bnn_mi355x_scan_clip_frames(const bnn_mi355x_frames *frames, const void *pixels, const int *sizes, int n_sizes, int number_class, int *boxes_out,
                                 float *usecPerImage, float *usecPreprocess, int enable_detail) {
  return scan_clip_call(frames_request("scan_clip_frames", pixels, frames, false, nullptr), sizes, n_sizes, number_class, boxes_out, usecPerImage,
                        usecPreprocess, enable_detail);
}

int *bnn_mi355x_scan_clip_device(const bnn_mi355x_frames *frames, const void *d_pixels, const int *sizes, int n_sizes, int number_class, int *boxes_out,
                                 float *usecPerImage, float *usecPreprocess, int enable_detail, void *hip_stream) {
  return scan_clip_call(frames_request("scan_clip_device", d_pixels, frames, true, hip_stream), sizes, n_sizes, number_class, boxes_out, usecPerImage,
                        usecPreprocess, enable_detail);
}

int bnn_mi355x_unpack_frames_host(const bnn_mi355x_frames *frames, const void *pixels, uint8_t *rgb_out) {
  PixLayout layout;
  const std::string bad = validate_frames("unpack_frames_host", reinterpret_cast<const Frames *>(frames), pixels, layout);
  if (!bad.empty()) return fail(bad);
  if (!rgb_out) return fail("unpack_frames_host: rgb_out is null");
  unpack_frames(*reinterpret_cast<const Frames *>(frames), layout, static_cast<const uint8_t *>(pixels), rgb_out);
  return 0;
}

int bnn_mi355x_unpack_frames(const bnn_mi355x_frames *frames, const void *pixels, uint8_t *rgb_out, float *usecUnpack) {
  Runtime &r = rt();
  if (usecUnpack) *usecUnpack = 0.f;
  if (!r.spec.is_cnv) return fail("unpack_frames: frames are unpacked on the device for the CNV networks only");
  PixLayout layout;
  const std::string bad = validate_frames("unpack_frames", reinterpret_cast<const Frames *>(frames), pixels, layout);
  if (!bad.empty()) return fail(bad);
  if (!rgb_out) return fail("unpack_frames: rgb_out is null");
  const Frames &f = *reinterpret_cast<const Frames *>(frames);
  if (bind_device()) return -1;
  // the RGB frames lie between two guards of kGuard bytes, which the kernel must leave as they were
  constexpr size_t kGuard = 64;
  const size_t rgb_bytes = (size_t)f.width * f.height * 3 * (size_t)f.n_frames;
  uint8_t guards[2 * kGuard];
  if (r.d_clip_raw.grow(layout.frame_span * (size_t)f.n_frames) || r.d_scan_scene.grow(rgb_bytes + 2 * kGuard) || ensure_events(r.pix_ev, 2)) return -1;
  DrainOnFailure drain;  // (declared after the host buffers the queued copies read or write)
  if (upload_raw(r.d_clip_raw, static_cast<const uint8_t *>(pixels), layout, r.stream)) return -1;
  uint8_t *const d_rgb = r.d_scan_scene + kGuard;
  HIP_OK(hipMemsetAsync(r.d_scan_scene, 0xA5, kGuard, r.stream));
  HIP_OK(hipMemsetAsync(d_rgb + rgb_bytes, 0xA5, kGuard, r.stream));
  UnpackLaunch u{};
  u.src = r.d_clip_raw; u.dst = d_rgb; u.frames = f; u.layout = uploaded_layout(layout); u.stream = r.stream;
  HIP_OK(hipEventRecord(r.pix_ev[0], r.stream));
  const hipError_t e = run_unpack_frames(u);
  if (e != hipSuccess) return launch_failed("unpack_frames", e);
  HIP_OK(hipEventRecord(r.pix_ev[1], r.stream));
  HIP_OK(hipMemcpyAsync(rgb_out, d_rgb, rgb_bytes, hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipMemcpyAsync(guards, r.d_scan_scene, kGuard, hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipMemcpyAsync(guards + kGuard, d_rgb + rgb_bytes, kGuard, hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  drain.ok();
  for (uint8_t g : guards)
    if (g != 0xA5) return fail("unpack_frames: internal: the kernel wrote outside the RGB frames");
  return usec_per_image(r.pix_ev[0], r.pix_ev[1], (size_t)f.n_frames, usecUnpack);
}

long bnn_mi355x_debug_scan_clip_stage(const uint8_t *pixels, int n_frames, long frame_stride, int width, int height, int bands, long row_stride,
                                      const int *sizes, int n_sizes, int stage, void *out, size_t cap) {
  Runtime &r = rt();
  const std::string no = scan_refused("debug_scan_clip_stage");
  if (!no.empty()) return fail(no);
  if (!out || stage < 0 || stage >= kScanStages) return fail("debug_scan_clip_stage: bad arguments");
  ClipPlan plan;
  const std::string bad = plan_clip("debug_scan_clip_stage", pixels, n_frames, frame_stride, width, height, bands, row_stride, sizes, n_sizes, out, plan);
  if (!bad.empty()) return fail(bad);
  const size_t bytes = plan.stage_bytes[stage];
  if (cap < bytes) return fail("debug_scan_clip_stage: the stage's maps take " + std::to_string(bytes) + " bytes");
  if (!ready() || bind_device()) return -1;
  ClipJob job;
  if (reserve_clip(plan, job)) return -1;
  DrainOnFailure drain;
  ClipSource src;
  src.pixels = pixels; src.stream = r.stream;
  if (enqueue_clip("debug_scan_clip_stage", plan, job, src, 1, nullptr, nullptr, nullptr, stage)) return -1;
  HIP_OK(hipMemcpyAsync(out, (stage & 1) ? r.d_scan_buf1 : r.d_scan_buf0, bytes, hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  drain.ok();
  return (long)bytes;
}

}  // extern "C"

// ---- detections: threshold, top-K and non-maximum suppression on the windows of a scan (CNV; detect.h) ----------------
namespace bnn {
namespace {

static_assert(sizeof(DetectOpts) == sizeof(bnn_mi355x_detect_opts) && offsetof(DetectOpts, max_det) == offsetof(bnn_mi355x_detect_opts, max_det),
              "DetectOpts is bnn_mi355x_detect_opts");
static_assert(kDetectMaxCandidates == BNN_MI355X_DETECT_MAX_CANDIDATES && kDetectMaxWindows == BNN_MI355X_SCAN_MAX_WINDOWS &&
                  kDetectMaxFrames == BNN_MI355X_SCAN_CLIP_MAX_FRAMES,
              "the header states the detections' limits");

// the workspaces of one detection call (grow-only) and one frame's boxes as the kernels hold them
int reserve_detect(const int *boxes, size_t n, int frames, const DetectOpts &o, std::vector<uint64_t> &packed) {
  Runtime &r = rt();
  packed.resize(n);
  for (size_t i = 0; i < n; i++) packed[i] = detect_pack_box(boxes + 4 * i);
  return (r.d_det_keys.grow(n * frames) || r.d_det_boxes.grow(n) || r.d_det_out.grow((size_t)frames * ((size_t)o.max_det * kDetectFields + 2)) ||
          ensure_events(r.det_ev, 2))
             ? -1 : 0;
}

// Enqueues on s: the upload of the boxes, the two detection launches between det_ev[0] and det_ev[1] on the scores
// (and classes, when the decode left them) of frames x n windows in HBM, and the lists' way back.  `packed` outlives the call's wait.
int enqueue_detect(const char *what, const std::vector<uint64_t> &packed, int frames, int ncls, const DetectOpts &o, const int16_t *d_scores,
                   const int32_t *d_classes, int *dets, int *counts, int *n_candidates, hipStream_t s) {
  Runtime &r = rt();
  const size_t n = packed.size(), det_ints = (size_t)frames * o.max_det * kDetectFields;
  if (n * frames > r.d_det_keys.cap || n > r.d_det_boxes.cap || det_ints + 2 * (size_t)frames > r.d_det_out.cap)
    return fail(std::string(what) + ": internal: the call exceeds the detection workspace");
  HIP_OK(hipMemcpyAsync(r.d_det_boxes, packed.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  HIP_OK(hipEventRecord(r.det_ev[0], s));
  DetectLaunch a{};
  a.scores = d_scores; a.classes = d_classes; a.boxes = r.d_det_boxes; a.keys = r.d_det_keys;
  a.dets = r.d_det_out; a.counts = r.d_det_out + det_ints; a.n_candidates = r.d_det_out + det_ints + frames;
  a.n = (int)n; a.frames = frames; a.number_class = ncls; a.opts = o; a.stream = s;
  const hipError_t e = run_detect(a);
  if (e != hipSuccess) return launch_failed(what, e);
  HIP_OK(hipEventRecord(r.det_ev[1], s));
  HIP_OK(hipMemcpyAsync(dets, a.dets, det_ints * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(counts, a.counts, (size_t)frames * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(n_candidates, a.n_candidates, (size_t)frames * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  return 0;
}

// bnn_mi355x_detect_clip, _detect_clip_frames and _detect_clip_device (a device call: as scan_clip_call)
int detect_clip_call(const ClipRequest &q, const int *sizes, int n_sizes, int number_class, const bnn_mi355x_detect_opts *opts, int *dets, int *counts,
                     int *n_candidates, float *usecPerImage, float *usecPreprocess, float *usecDetect) {
  Runtime &r = rt();
  const std::string name = std::string(q.what) + ": ";
  if (usecPerImage) *usecPerImage = 0.f;
  if (usecPreprocess) *usecPreprocess = 0.f;
  if (usecDetect) *usecDetect = 0.f;
  const std::string no = scan_refused(q.what);
  if (!no.empty()) return fail(no);
  ClipPlan plan;
  ClipSource src;
  // (plan_clip refuses a null boxes_out: the boxes stay in this call, dets stands in for the check)
  const std::string bad = plan_request(q, sizes, n_sizes, dets, plan, src);
  if (!bad.empty()) return fail(bad);
  if (!dets) return fail(name + "dets is null");
  if (!counts) return fail(name + "counts is null");
  if (!n_candidates) return fail(name + "n_candidates is null");
  const DetectOpts *o = reinterpret_cast<const DetectOpts *>(opts);
  const std::string bad_opts = validate_detect_opts(q.what, number_class, o);
  if (!bad_opts.empty()) return fail(bad_opts);
  if (!ready()) return -1;
  const std::string captured = capture_refused(q);
  if (!captured.empty()) return fail(captured);
  const size_t windows = (size_t)plan.windows, n = windows / (size_t)plan.frames;
  std::vector<int> boxes(4 * n);
  for (const ScanLevel &lv : plan.scene.levels)
    scan_boxes(plan.width, plan.height, lv.size, boxes.data() + 4 * (size_t)lv.first, (long)lv.plan.nx * lv.plan.ny);
  if (bind_device()) return -1;
  const hipStream_t s = src.stream = q.device ? static_cast<hipStream_t>(q.hip_stream) : r.stream;
  ClipJob job;  // (outlives its asynchronous uploads: declared before `drain`)
  std::vector<uint64_t> packed;
  // every workspace first (they synchronise when they grow), so that nothing is allocated between the kernels
  if (reserve_results(windows) || reserve_clip(plan, job, src.raw_bytes()) || reserve_detect(boxes.data(), n, plan.frames, *o, packed) ||
      ensure_events(r.scan_ev, 3))
    return -1;
  DrainOnFailure drain;
  DrainCaller caller{src};
  HIP_OK(hipEventRecord(r.scan_ev[0], s));
  if (enqueue_clip(q.what, plan, job, src, number_class, r.d_classes, r.d_scores, r.scan_ev[1], kCnvStages - 1)) return -1;
  HIP_OK(hipEventRecord(r.scan_ev[2], s));
  if (enqueue_detect(q.what, packed, plan.frames, number_class, *o, r.d_scores, r.d_classes, dets, counts, n_candidates, s)) return -1;
  HIP_OK(hipStreamSynchronize(s));
  drain.ok();
  caller.ok();
  return (usec_per_image(r.scan_ev[0], r.scan_ev[1], windows, usecPreprocess) || usec_per_image(r.scan_ev[1], r.scan_ev[2], windows, usecPerImage) ||
          usec_per_image(r.det_ev[0], r.det_ev[1], (size_t)plan.frames, usecDetect))
             ? -1 : 0;
}

}  // namespace
}  // namespace bnn

extern "C" {

int bnn_mi355x_detect_windows_host(const int *boxes, int n, const int *scores, int frames, int number_class, const bnn_mi355x_detect_opts *opts,
                                   int *dets, int *counts, int *n_candidates) {
  const DetectOpts *o = reinterpret_cast<const DetectOpts *>(opts);
  const std::string bad = validate_detect("detect_windows_host", boxes, n, scores, frames, number_class, o, dets, counts, n_candidates);
  if (!bad.empty()) return fail(bad);
  detect_windows(boxes, n, scores, frames, number_class, *o, dets, counts, n_candidates);
  return 0;
}

int bnn_mi355x_detect_windows(const int *boxes, int n, const int *scores, int frames, int number_class, const bnn_mi355x_detect_opts *opts,
                              int *dets, int *counts, int *n_candidates, float *usecDetect) {
  Runtime &r = rt();
  if (usecDetect) *usecDetect = 0.f;
  if (!r.spec.is_cnv) return fail("detect_windows: the scores of a window are the output of the CNV networks only");
  const DetectOpts *o = reinterpret_cast<const DetectOpts *>(opts);
  const std::string bad = validate_detect("detect_windows", boxes, n, scores, frames, number_class, o, dets, counts, n_candidates);
  if (!bad.empty()) return fail(bad);
  if (bind_device()) return -1;
  // the scores as the decode kernels leave them: 64 int16 a window
  const size_t windows = (size_t)n * frames;
  std::vector<int16_t> rows(windows * 64, 0);
  for (size_t i = 0; i < windows; i++)
    for (int c = 0; c < number_class; c++) rows[i * 64 + c] = (int16_t)scores[i * number_class + c];
  std::vector<uint64_t> packed;
  if (reserve_detect(boxes, (size_t)n, frames, *o, packed) || r.d_det_scores.grow(windows * 64)) return -1;
  DrainOnFailure drain;  // (declared after the host buffers the queued copies read or write)
  HIP_OK(hipMemcpyAsync(r.d_det_scores, rows.data(), rows.size() * sizeof(int16_t), hipMemcpyHostToDevice, r.stream));
  if (enqueue_detect("detect_windows", packed, frames, number_class, *o, r.d_det_scores, nullptr, dets, counts, n_candidates, r.stream)) return -1;
  HIP_OK(hipStreamSynchronize(r.stream));
  drain.ok();
  return usec_per_image(r.det_ev[0], r.det_ev[1], (size_t)frames, usecDetect);
}

int bnn_mi355x_detect_clip(const uint8_t *pixels, int n_frames, long frame_stride, int width, int height, int bands, long row_stride,
                           const int *sizes, int n_sizes, int number_class, const bnn_mi355x_detect_opts *opts, int *dets, int *counts,
                           int *n_candidates, float *usecPerImage, float *usecPreprocess, float *usecDetect) {
  const ClipRequest q{"detect_clip", pixels, false, nullptr, n_frames, frame_stride, width, height, bands, row_stride, false, nullptr};
  return detect_clip_call(q, sizes, n_sizes, number_class, opts, dets, counts, n_candidates, usecPerImage, usecPreprocess, usecDetect);
}

int bnn_mi355x_detect_clip_frames(const bnn_mi355x_frames *frames, const void *pixels, const int *sizes, int n_sizes, int number_class,
                                  const bnn_mi355x_detect_opts *opts, int *dets, int *counts, int *n_candidates, float *usecPerImage,
                                  float *usecPreprocess, float *usecDetect) {
  return detect_clip_call(frames_request("detect_clip_frames", pixels, frames, false, nullptr), sizes, n_sizes, number_class, opts, dets, counts,
                          n_candidates, usecPerImage, usecPreprocess, usecDetect);
}

int bnn_mi355x_detect_clip_device(const bnn_mi355x_frames *frames, const void *d_pixels, const int *sizes, int n_sizes, int number_class,
                                  const bnn_mi355x_detect_opts *opts, int *dets, int *counts, int *n_candidates, float *usecPerImage,
                                  float *usecPreprocess, float *usecDetect, void *hip_stream) {
  return detect_clip_call(frames_request("detect_clip_device", d_pixels, frames, true, hip_stream), sizes, n_sizes, number_class, opts, dets, counts,
                          n_candidates, usecPerImage, usecPreprocess, usecDetect);
}

}  // extern "C"

// ---- one picture and N boxes -> MNIST-format records / classes (LFC; glyphs.h) ----------------------------------
namespace bnn {
namespace {

static_assert(sizeof(GlyphDesc) == 16 * sizeof(int32_t), "the record kernel reads a glyph's descriptor as 16 ints");
static_assert(kGlyphMidBytes == BNN_MI355X_GLYPH_LDS_BYTES && kGlyphMidBytes + kGlyphRecord <= 65536, "the header states the record kernel's LDS bound");
static_assert(kGlyphRecord % 16 == 0, "records are written with 16-byte stores");

GlyphOpts glyph_opts(const bnn_mi355x_glyph_opts *o) {
  GlyphOpts g;
  if (o) { g.contrast = o->contrast; g.brightness = o->brightness; g.threshold = o->threshold; g.filter = o->filter; g.square_blank = o->square_blank; }
  return g;
}

// Enqueues, on r.stream: the picture's upload (rows padded to whole 16-pixel lanes), k_glyph_luma and -- when a step is
// not the identity -- k_glyph_enhance.  Afterwards p.plane is the enhanced L plane and *p.sum the pixel sum of the plane
// before the enhancement.  The caller has validated the arguments and bound the device.
int enqueue_glyph_plane(const char *what, const uint8_t *pixels, int width, int height, int bands, long row_stride, const GlyphOpts &o,
                        GlyphPicture &p) {
  Runtime &r = rt();
  const long pitch = glyph_plane_pitch(width);
  const size_t src_pitch = (size_t)pitch * bands, row_bytes = (size_t)width * bands;
  if (r.d_gl_src.grow(src_pitch * height) || r.d_gl_plane.grow((size_t)pitch * height) || r.d_gl_sum.grow(1)) return -1;
  HIP_OK(hipMemcpy2DAsync(r.d_gl_src, src_pitch, pixels, row_stride ? (size_t)row_stride : row_bytes, row_bytes, (size_t)height, hipMemcpyHostToDevice,
                          r.stream));
  HIP_OK(hipMemsetAsync(r.d_gl_sum, 0, sizeof(unsigned long long), r.stream));
  p = GlyphPicture{};
  p.src = r.d_gl_src; p.plane = r.d_gl_plane; p.width = width; p.height = height; p.bands = bands; p.plane_pitch = pitch; p.sum = r.d_gl_sum;
  hipError_t e = launch_glyph_luma(p, r.stream);
  if (e == hipSuccess && (o.contrast != 1.0f || o.brightness != 1.0f || o.threshold >= 0))
    e = launch_glyph_enhance(p, o.contrast, o.brightness, o.threshold, r.stream);
  if (e != hipSuccess) return launch_failed(what, e);
  return 0;
}

// Behind enqueue_glyph_plane: one upload of the boxes, k_glyph_bbox, the call's ONE host round trip (the n x 4 ink boxes
// come back, the fit and the tables are made from them, descriptors and tables go up in one upload), k_glyph_record.
// Record i lands at r.d_gl_rec + i * 784; `plan` holds status and ink boxes.  `meta` outlives its uploads.
int enqueue_glyph_records(const char *what, const GlyphPicture &p, const int *boxes, int n, const GlyphOpts &o, GlyphPlan &plan,
                          std::vector<int32_t> &meta) {
  Runtime &r = rt();
  const size_t off_found = (size_t)n * 4;
  meta.assign((size_t)n * 8, 0);
  std::memcpy(meta.data(), boxes, (size_t)n * 4 * sizeof(int32_t));
  int tallest = 1;
  for (int i = 0; i < n; i++) {
    int32_t *f = meta.data() + off_found + 4 * (size_t)i;
    f[0] = f[1] = INT_MAX;
    f[2] = f[3] = -1;
    tallest = std::max(tallest, boxes[4 * (size_t)i + 3] - boxes[4 * (size_t)i + 1]);
  }
  if (r.d_gl_box.grow(meta.size()) || r.d_gl_rec.grow((size_t)n * kGlyphRecord) || r.d_gl_plan.grow((size_t)n * 16 + 4096)) return -1;
  HIP_OK(hipMemcpyAsync(r.d_gl_box, meta.data(), meta.size() * sizeof(int32_t), hipMemcpyHostToDevice, r.stream));
  hipError_t e = launch_glyph_bbox(p, r.d_gl_box, r.d_gl_box + off_found, n, tallest, r.stream);
  if (e != hipSuccess) return launch_failed(what, e);
  std::vector<int32_t> found((size_t)n * 4);
  HIP_OK(hipMemcpyAsync(found.data(), r.d_gl_box + off_found, found.size() * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  const std::string bad = plan_glyphs(boxes, found.data(), n, o.filter, o.square_blank, plan);
  if (!bad.empty()) return fail(std::string(what) + ": " + bad);
  const size_t off_coef = (size_t)n * 16;
  meta.assign(off_coef + plan.coef.size(), 0);
  std::memcpy(meta.data(), plan.desc.data(), (size_t)n * sizeof(GlyphDesc));
  if (!plan.coef.empty()) std::memcpy(meta.data() + off_coef, plan.coef.data(), plan.coef.size() * sizeof(int32_t));
  // (the stream is idle here: growing costs no second wait)
  if (r.d_gl_plan.grow(meta.size()) || (plan.tmp_bytes && r.d_gl_tmp.grow(plan.tmp_bytes))) return -1;
  HIP_OK(hipMemcpyAsync(r.d_gl_plan, meta.data(), meta.size() * sizeof(int32_t), hipMemcpyHostToDevice, r.stream));
  e = launch_glyph_record(p, reinterpret_cast<const GlyphDesc *>(r.d_gl_plan.get()), r.d_gl_plan + off_coef, plan.tmp_bytes ? r.d_gl_tmp : nullptr,
                          r.d_gl_rec, n, r.stream);
  if (e != hipSuccess) return launch_failed(what, e);
  return 0;
}

const char kGlyphsLfcOnly[] = ": MNIST-format records are the input of the LFC networks only";

}  // namespace
}  // namespace bnn

extern "C" {

int bnn_mi355x_glyph_fit(int width, int height, int out[5]) {
  const GlyphFit f = glyph_fit(width, height);
  if (out) { out[0] = f.out_w; out[1] = f.out_h; out[2] = f.off_x; out[3] = f.off_y; out[4] = f.status; }
  return f.status;
}

int bnn_mi355x_resample_coeffs(int filter, int in_size, int out_size, int *kk, int *bounds, int cap_kk) {
  std::vector<int32_t> k, b;
  const int ksize = resample_coeffs(filter, in_size, out_size, k, b);
  if (ksize <= 0) return fail("resample_coeffs: need filter 0 (NEAREST) or 3 (BICUBIC) and sizes of 1 or more");
  if (kk && cap_kk > 0 && (size_t)cap_kk >= k.size()) std::memcpy(kk, k.data(), k.size() * sizeof(int32_t));
  if (bounds) std::memcpy(bounds, b.data(), b.size() * sizeof(int32_t));
  return ksize;
}

int bnn_mi355x_enhance_picture(const uint8_t *pixels, int width, int height, int bands, long row_stride, const bnn_mi355x_glyph_opts *opts,
                               uint8_t *out_L, int *out_mean) {
  Runtime &r = rt();
  if (r.spec.is_cnv) return fail(std::string("enhance_picture") + kGlyphsLfcOnly);
  const GlyphOpts o = glyph_opts(opts);
  const std::string bad = validate_glyphs("enhance_picture", pixels, width, height, bands, row_stride, nullptr, 0, opts ? &o : nullptr, out_L);
  if (!bad.empty()) return fail(bad);
  if (bind_device()) return -1;
  DrainOnFailure drain;
  GlyphPicture p;
  if (enqueue_glyph_plane("enhance_picture", pixels, width, height, bands, row_stride, o, p)) return -1;
  unsigned long long sum = 0;
  HIP_OK(hipMemcpy2DAsync(out_L, (size_t)width, p.plane, (size_t)p.plane_pitch, (size_t)width, (size_t)height, hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipMemcpyAsync(&sum, p.sum, sizeof sum, hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  drain.ok();
  const unsigned long long n = (unsigned long long)width * (unsigned long long)height;
  if (out_mean) *out_mean = (int)((2 * sum + n) / (2 * n));
  return 0;
}

int bnn_mi355x_glyphs_to_mnist(const uint8_t *pixels, int width, int height, int bands, long row_stride, const int *boxes, int n_boxes,
                               const bnn_mi355x_glyph_opts *opts, uint8_t *records, int *ink_boxes, int *status) {
  Runtime &r = rt();
  if (r.spec.is_cnv) return fail(std::string("glyphs_to_mnist") + kGlyphsLfcOnly);
  const GlyphOpts o = glyph_opts(opts);
  const std::string bad = validate_glyphs("glyphs_to_mnist", pixels, width, height, bands, row_stride, boxes, n_boxes, opts ? &o : nullptr, records);
  if (!bad.empty()) return fail(bad);
  const int whole[4] = {0, 0, width, height};
  if (!boxes || n_boxes == 0) { boxes = whole; n_boxes = 1; }
  const int n = n_boxes;
  if (bind_device()) return -1;
  GlyphPlan plan;
  std::vector<int32_t> meta;
  DrainOnFailure drain;
  GlyphPicture p;
  if (enqueue_glyph_plane("glyphs_to_mnist", pixels, width, height, bands, row_stride, o, p) ||
      enqueue_glyph_records("glyphs_to_mnist", p, boxes, n, o, plan, meta) || download_glyph_records((size_t)n, plan.status, records, status))
    return -1;
  drain.ok();
  if (ink_boxes) std::memcpy(ink_boxes, plan.ink_boxes.data(), (size_t)n * 4 * sizeof(int32_t));
  return 0;
}

int *bnn_mi355x_classify_glyphs(const uint8_t *pixels, int width, int height, int bands, long row_stride, const int *boxes, int n_boxes,
                                const bnn_mi355x_glyph_opts *opts, int number_class, float *usecPerImage, float *usecPreprocess, int *status) {
  Runtime &r = rt();
  if (usecPerImage) *usecPerImage = 0.f;
  if (usecPreprocess) *usecPreprocess = 0.f;
  if (r.spec.is_cnv) { fail(std::string("classify_glyphs") + kGlyphsLfcOnly); return nullptr; }
  const GlyphOpts o = glyph_opts(opts);
  // (no output buffer of the caller's to check: the result array is the call's own)
  const std::string bad = validate_glyphs("classify_glyphs", pixels, width, height, bands, row_stride, boxes, n_boxes, opts ? &o : nullptr, pixels);
  if (!bad.empty()) { fail(bad); return nullptr; }
  if (bad_number_class(number_class)) return nullptr;
  const int whole[4] = {0, 0, width, height};
  if (!boxes || n_boxes == 0) { boxes = whole; n_boxes = 1; }
  const int n = n_boxes;
  if (!ready()) return nullptr;
  int *result = new_result((size_t)n);
  if (!result) return nullptr;
  // everything that can fail from here on frees `result`
  auto run = [&]() -> int {
    if (bind_device()) return -1;
    GlyphPlan plan;
    std::vector<int32_t> meta;
    // the pass's workspaces first (they synchronise when they grow), so that nothing is allocated between the kernels
    if (reserve_results((size_t)n) || ensure_events(r.gl_ev, 3)) return -1;
    DrainOnFailure drain;
    GlyphPicture p;
    HIP_OK(hipEventRecord(r.gl_ev[0], r.stream));
    if (enqueue_glyph_plane("classify_glyphs", pixels, width, height, bands, row_stride, o, p) ||
        enqueue_glyph_records("classify_glyphs", p, boxes, n, o, plan, meta) || classify_glyph_records(n, number_class, plan.status, result, status))
      return -1;
    drain.ok();
    return (usec_per_image(r.gl_ev[0], r.gl_ev[1], (size_t)n, usecPreprocess) || usec_per_image(r.gl_ev[1], r.gl_ev[2], (size_t)n, usecPerImage)) ? -1 : 0;
  };
  if (run()) { delete[] result; return nullptr; }
  return result;
}

}  // extern "C"

// ---- the glyphs of a picture: connected components of its ink (LFC; components.h) ----------------------------------
namespace bnn {
namespace {

static_assert(sizeof(Component) == 8 * sizeof(int32_t), "the kernels and the read-back take a component as 8 ints");
static_assert(kMaxComponentPixels == BNN_MI355X_FIND_MAX_PIXELS && kMaxReach == BNN_MI355X_FIND_MAX_REACH, "the header states the model's limits");

FindOpts find_opts(const bnn_mi355x_find_opts *f) {
  FindOpts o;
  if (f) { o.ink_level = f->ink_level; o.reach_x = f->reach_x; o.reach_y = f->reach_y; o.min_pixels = f->min_pixels; o.order = f->order; }
  return o;
}

constexpr size_t kFirstReadBack = 4096;  // components that come back with the counters, in the call's one copy

// The workspaces of a picture of width x height pixels, before anything is enqueued (growing synchronises).
int reserve_components(int width, int height, bool labels) {
  Runtime &r = rt();
  const size_t n = (size_t)width * height, comps = max_components(width, height);
  if (r.d_cc_bits.grow((size_t)height * cc_words_per_row(width)) || r.d_cc_label.grow(n) || r.d_cc_stat.grow(comps) ||
      r.d_cc_list.grow(kComponentHead + comps * 8) || (labels && (r.d_cc_index.grow(comps) || r.d_cc_out.grow(n))))
    return -1;
  return ensure_events(r.cc_ev, 2);
}

// Behind enqueue_glyph_plane, on r.stream: the six labelling launches, the call's round trip for the component list
// (the counters and the first kFirstReadBack components in one copy; a second copy only for more), select_components,
// and -- when `labels` is not null -- the index map's upload, k_cc_relabel and the map's copy into `labels`, which the
// caller waits for.  `chosen`: the returned components in order; `index` outlives its upload.
int enqueue_components(const char *what, const GlyphPicture &p, const FindOpts &f, int cap, int32_t *labels, std::vector<Component> &chosen,
                       long &total, std::vector<int32_t> &index) {
  Runtime &r = rt();
  const int comps = (int)max_components(p.width, p.height);
  ComponentPlane c{};
  c.plane = p.plane; c.plane_pitch = p.plane_pitch; c.width = p.width; c.height = p.height;
  c.words_per_row = cc_words_per_row(p.width); c.bits = r.d_cc_bits; c.label = r.d_cc_label;
  HIP_OK(hipEventRecord(r.cc_ev[0], r.stream));
  hipError_t e = launch_cc_label(c, f.ink_level, f.reach_x, f.reach_y, r.stream);
  if (e == hipSuccess) e = launch_cc_collect(c, r.d_cc_list, r.d_cc_stat, comps, f.min_pixels, r.stream);
  if (e != hipSuccess) return launch_failed(what, e);
  HIP_OK(hipEventRecord(r.cc_ev[1], r.stream));
  const size_t first = std::min((size_t)comps, kFirstReadBack);
  std::vector<int32_t> back(kComponentHead + first * 8);
  HIP_OK(hipMemcpyAsync(back.data(), r.d_cc_list, back.size() * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
  HIP_OK(hipStreamSynchronize(r.stream));
  const long roots = back[0], kept = back[1];
  if (roots < 0 || roots > comps || kept < 0 || kept > roots) return fail(std::string(what) + ": internal: the component counters are out of range");
  if ((size_t)kept > first) {
    back.resize(kComponentHead + (size_t)kept * 8);
    HIP_OK(hipMemcpyAsync(back.data(), r.d_cc_list, back.size() * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
    HIP_OK(hipStreamSynchronize(r.stream));
  }
  HIP_OK(hipEventElapsedTime(&r.cc_usec, r.cc_ev[0], r.cc_ev[1]));
  r.cc_usec *= 1000.f;
  std::vector<Component> all((size_t)kept);
  if (kept) std::memcpy(all.data(), back.data() + kComponentHead, (size_t)kept * sizeof(Component));
  for (const Component &k : all)
    if (k.id < 0 || k.id >= roots || k.left < 0 || k.upper < 0 || k.right > p.width || k.lower > p.height || k.left >= k.right || k.upper >= k.lower)
      return fail(std::string(what) + ": internal: a component's box leaves the picture");
  total = select_components(all, f, cap, chosen);
  if (labels) {
    index.assign((size_t)std::max(roots, 1L), -1);
    for (size_t k = 0; k < chosen.size(); k++) index[(size_t)chosen[k].id] = (int32_t)k;
    HIP_OK(hipMemcpyAsync(r.d_cc_index, index.data(), index.size() * sizeof(int32_t), hipMemcpyHostToDevice, r.stream));
    e = launch_cc_relabel(c, r.d_cc_index, r.d_cc_out, r.stream);
    if (e != hipSuccess) return launch_failed(what, e);
    HIP_OK(hipMemcpyAsync(labels, r.d_cc_out, (size_t)p.width * p.height * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
  }
  return 0;
}

void boxes_of(const std::vector<Component> &chosen, int *boxes, int *pixel_counts) {
  for (size_t k = 0; k < chosen.size(); k++) {
    const Component &c = chosen[k];
    boxes[4 * k] = c.left; boxes[4 * k + 1] = c.upper; boxes[4 * k + 2] = c.right; boxes[4 * k + 3] = c.lower;
    if (pixel_counts) pixel_counts[k] = c.pixels;
  }
}

}  // namespace
}  // namespace bnn

extern "C" {

int bnn_mi355x_find_glyphs_host(const uint8_t *plane, int width, int height, long row_stride, const bnn_mi355x_find_opts *find, int *boxes,
                                int *pixel_counts, int32_t *labels, int cap) {
  const FindOpts f = find_opts(find);
  const GlyphOpts o;
  std::string bad = validate_glyphs("find_glyphs_host", plane, width, height, 1, row_stride, nullptr, 0, &o, boxes);
  if (bad.empty()) bad = validate_find("find_glyphs_host", width, height, &f, boxes, cap);
  if (!bad.empty()) return fail(bad);
  const long total = find_components_host(plane, width, height, row_stride, f, boxes, pixel_counts, labels, cap);
  return (int)total;
}

float bnn_mi355x_last_find_usec(void) { return rt().cc_usec; }

int bnn_mi355x_find_glyphs(const uint8_t *pixels, int width, int height, int bands, long row_stride, const bnn_mi355x_glyph_opts *opts,
                           const bnn_mi355x_find_opts *find, int *boxes, int *pixel_counts, int32_t *labels, int cap) {
  Runtime &r = rt();
  if (r.spec.is_cnv) return fail(std::string("find_glyphs") + kGlyphsLfcOnly);
  const GlyphOpts o = glyph_opts(opts);
  const FindOpts f = find_opts(find);
  std::string bad = validate_glyphs("find_glyphs", pixels, width, height, bands, row_stride, nullptr, 0, opts ? &o : nullptr, boxes);
  if (bad.empty()) bad = validate_find("find_glyphs", width, height, &f, boxes, cap);
  if (!bad.empty()) return fail(bad);
  if (bind_device()) return -1;
  std::vector<Component> chosen;
  std::vector<int32_t> index;
  long total = 0;
  if (reserve_components(width, height, labels != nullptr)) return -1;
  DrainOnFailure drain;
  GlyphPicture p;
  if (enqueue_glyph_plane("find_glyphs", pixels, width, height, bands, row_stride, o, p) ||
      enqueue_components("find_glyphs", p, f, cap, labels, chosen, total, index))
    return -1;
  if (labels) HIP_OK(hipStreamSynchronize(r.stream));
  drain.ok();
  boxes_of(chosen, boxes, pixel_counts);
  return (int)total;
}

}  // extern "C"

// ---- a page: lines of text, glyphs masked to their own ink (LFC; page.h) --------------------------------------------
namespace bnn {
namespace {

static_assert(kMaxLineComponents == BNN_MI355X_PAGE_MAX_LINE_COMPONENTS, "the header states the line model's limit");

PageOpts page_opts(const bnn_mi355x_page_opts *g) {
  PageOpts o;
  if (g) { o.mask = g->mask; o.line_order = g->line_order; o.word_gap = g->word_gap; }
  return o;
}

struct Page {
  std::vector<Component> chosen;             // the returned glyphs in output order
  std::vector<int32_t> line, gap;            // per returned glyph
  std::vector<int32_t> index, meta, found;   // uploads and boxes that outlive the enqueue
  GlyphPlan plan;
  long total = 0;
};

// The masked route behind the component list, with NO further round trip: descriptors, keys and tables go up in one
// upload, then k_page_record.  Record i lands at r.d_gl_rec + i * 784.  The stream is idle when this is called (the
// component list has just come back): growing costs no second wait.
int enqueue_page_records(const char *what, const GlyphPicture &p, const GlyphOpts &o, Page &pg) {
  Runtime &r = rt();
  const size_t n = pg.chosen.size();
  std::vector<int32_t> keys;
  const std::string bad = plan_page(pg.chosen, o.filter, o.square_blank, pg.plan, keys);
  if (!bad.empty()) return fail(std::string(what) + ": " + bad);
  const size_t off_keys = n * 16, off_coef = off_keys + n * 2;
  pg.meta.assign(off_coef + pg.plan.coef.size(), 0);
  std::memcpy(pg.meta.data(), pg.plan.desc.data(), n * sizeof(GlyphDesc));
  std::memcpy(pg.meta.data() + off_keys, keys.data(), keys.size() * sizeof(int32_t));
  if (!pg.plan.coef.empty()) std::memcpy(pg.meta.data() + off_coef, pg.plan.coef.data(), pg.plan.coef.size() * sizeof(int32_t));
  if (r.d_gl_plan.grow(pg.meta.size()) || r.d_gl_rec.grow(n * kGlyphRecord) || (pg.plan.tmp_bytes && r.d_gl_tmp.grow(pg.plan.tmp_bytes))) return -1;
  HIP_OK(hipMemcpyAsync(r.d_gl_plan, pg.meta.data(), pg.meta.size() * sizeof(int32_t), hipMemcpyHostToDevice, r.stream));
  const hipError_t e = launch_page_record(p, r.d_cc_label, reinterpret_cast<const GlyphDesc *>(r.d_gl_plan.get()), r.d_gl_plan + off_keys,
                                          r.d_gl_plan + off_coef, pg.plan.tmp_bytes ? r.d_gl_tmp : nullptr, r.d_gl_rec, (int)n, r.stream);
  if (e != hipSuccess) return launch_failed(what, e);
  return 0;
}

// Upload, enhance, label, collect, the component list's round trip, the order (select_components' result, put into lines
// when asked for, then the cap) and the records: k_page_record under the mask, else exactly read_glyphs' sequence on the
// ordered boxes.  `classify`: the pass's workspaces are reserved while the stream is idle.  With no glyph nothing is
// enqueued behind the round trip.  `total_early` (read_glyphs' n_found; may be null) is written as soon as the component
// list is back.
int enqueue_page(const char *what, const uint8_t *pixels, int width, int height, int bands, long row_stride, const GlyphOpts &o, const FindOpts &f,
                 const PageOpts &g, int cap, bool classify, Page &pg, int *total_early = nullptr) {
  GlyphPicture p;
  if (enqueue_glyph_plane(what, pixels, width, height, bands, row_stride, o, p) ||
      enqueue_components(what, p, f, g.line_order ? INT_MAX : cap, nullptr, pg.chosen, pg.total, pg.index))
    return -1;
  if (total_early) *total_early = (int)pg.total;
  if (g.line_order) {
    std::vector<int32_t> order;
    const std::string bad = order_lines(pg.chosen, g.word_gap, order, pg.line, pg.gap);
    if (!bad.empty()) return fail(std::string(what) + ": " + bad);
    const size_t n = std::min(order.size(), (size_t)cap);
    std::vector<Component> ordered(n);
    for (size_t i = 0; i < n; i++) ordered[i] = pg.chosen[(size_t)order[i]];
    pg.chosen.swap(ordered);
    pg.line.resize(n);
    pg.gap.resize(n);
  } else {
    pg.line.assign(pg.chosen.size(), 0);
    pg.gap.assign(pg.chosen.size(), 0);
  }
  const int n = (int)pg.chosen.size();
  pg.found.resize((size_t)n * 4);
  boxes_of(pg.chosen, pg.found.data(), nullptr);
  if (n == 0) return 0;
  if (classify && reserve_results((size_t)n)) return -1;
  if (g.mask) return enqueue_page_records(what, p, o, pg);
  return enqueue_glyph_records(what, p, pg.found.data(), n, o, pg.plan, pg.meta);
}

// (g null: read_glyphs, which has no page options to refuse)
std::string validate_page_call(const char *what, const uint8_t *pixels, int width, int height, int bands, long row_stride, const GlyphOpts *o,
                               const FindOpts &f, const PageOpts *g, const void *n_found, const void *boxes, int cap) {
  std::string bad = validate_glyphs(what, pixels, width, height, bands, row_stride, nullptr, 0, o, n_found);
  if (bad.empty()) bad = validate_find(what, width, height, &f, boxes, cap);
  if (bad.empty() && g) bad = validate_page(what, g);
  return bad;
}

// bnn_mi355x_read_page, and bnn_mi355x_read_glyphs as the page with no mask and no line order (`page` null: its options are
// not the caller's to get wrong, n_found is written as soon as the glyphs are counted, line and gap are null)
int *read_page(const char *what, const uint8_t *pixels, int width, int height, int bands, long row_stride, const bnn_mi355x_glyph_opts *opts,
               const bnn_mi355x_find_opts *find, const PageOpts *page, int number_class, int cap, int *n_found, int *boxes, int *line, int *gap,
               float *usecPerImage, float *usecPreprocess, int *status) {
  Runtime &r = rt();
  if (usecPerImage) *usecPerImage = 0.f;
  if (usecPreprocess) *usecPreprocess = 0.f;
  if (r.spec.is_cnv) { fail(std::string(what) + kGlyphsLfcOnly); return nullptr; }
  const GlyphOpts o = glyph_opts(opts);
  const FindOpts f = find_opts(find);
  const PageOpts g = page ? *page : PageOpts{0, 0, 0};
  const std::string bad = validate_page_call(what, pixels, width, height, bands, row_stride, opts ? &o : nullptr, f, page, n_found, boxes, cap);
  if (!bad.empty()) { fail(bad); return nullptr; }
  if (bad_number_class(number_class) || !ready()) return nullptr;
  int *result = nullptr;
  // everything that can fail from here on frees `result`
  auto run = [&]() -> int {
    if (bind_device()) return -1;
    Page pg;
    if (reserve_components(width, height, false) || ensure_events(r.gl_ev, 3)) return -1;
    DrainOnFailure drain;
    HIP_OK(hipEventRecord(r.gl_ev[0], r.stream));
    if (enqueue_page(what, pixels, width, height, bands, row_stride, o, f, g, cap, true, pg, page ? nullptr : n_found)) return -1;
    const int n = (int)pg.chosen.size();
    if (!(result = new_result((size_t)n))) return -1;
    *n_found = (int)pg.total;
    if (n == 0) {  // nothing to read: a non-null, empty result
      HIP_OK(hipStreamSynchronize(r.stream));
      drain.ok();
      return 0;
    }
    if (classify_glyph_records(n, number_class, pg.plan.status, result, status)) return -1;
    drain.ok();
    for (int i = 0; i < n; i++) {
      if (line) line[i] = pg.line[(size_t)i];
      if (gap) gap[i] = pg.gap[(size_t)i];
    }
    std::memcpy(boxes, pg.found.data(), pg.found.size() * sizeof(int));
    return (usec_per_image(r.gl_ev[0], r.gl_ev[1], (size_t)n, usecPreprocess) || usec_per_image(r.gl_ev[1], r.gl_ev[2], (size_t)n, usecPerImage)) ? -1 : 0;
  };
  if (run()) { delete[] result; return nullptr; }
  return result;
}

}  // namespace
}  // namespace bnn

extern "C" {

int bnn_mi355x_order_lines(const int *boxes, const int *first, int n, int word_gap, int *order, int *line, int *gap) {
  const std::string bad = validate_order_lines("order_lines", boxes, first, n, word_gap, order);
  if (!bad.empty()) return fail(bad);
  std::vector<Component> kept((size_t)n);
  for (int i = 0; i < n; i++) {
    const int *b = boxes + 4 * (size_t)i;
    kept[(size_t)i] = Component{first[i], b[0], b[1], b[2], b[3], 1, first[i], 0};
  }
  std::vector<int32_t> o, l, g;
  const std::string refused = order_lines(kept, word_gap, o, l, g);
  if (!refused.empty()) return fail("order_lines: " + refused);
  for (int i = 0; i < n; i++) {
    order[i] = o[(size_t)i];
    if (line) line[i] = l[(size_t)i];
    if (gap) gap[i] = g[(size_t)i];
  }
  return 0;
}

int bnn_mi355x_page_to_mnist(const uint8_t *pixels, int width, int height, int bands, long row_stride, const bnn_mi355x_glyph_opts *opts,
                             const bnn_mi355x_find_opts *find, const bnn_mi355x_page_opts *page, int cap, int *n_found, int *boxes,
                             uint8_t *records, int *status, int *line, int *gap) {
  Runtime &r = rt();
  if (r.spec.is_cnv) return fail(std::string("page_to_mnist") + kGlyphsLfcOnly);
  const GlyphOpts o = glyph_opts(opts);
  const FindOpts f = find_opts(find);
  const PageOpts g = page_opts(page);
  // (two outputs of the caller's that must not be null, one test: n_found stands for both)
  const std::string bad = validate_page_call("page_to_mnist", pixels, width, height, bands, row_stride, opts ? &o : nullptr, f, &g,
                                             records ? n_found : nullptr, boxes, cap);
  if (!bad.empty()) return fail(bad);
  if (bind_device()) return -1;
  Page pg;
  if (reserve_components(width, height, false)) return -1;
  DrainOnFailure drain;
  if (enqueue_page("page_to_mnist", pixels, width, height, bands, row_stride, o, f, g, cap, false, pg)) return -1;
  const size_t n = pg.chosen.size();
  if (download_glyph_records(n, pg.plan.status, records, status)) return -1;
  drain.ok();
  *n_found = (int)pg.total;
  for (size_t i = 0; i < n; i++) {
    if (line) line[i] = pg.line[i];
    if (gap) gap[i] = pg.gap[i];
  }
  if (n) std::memcpy(boxes, pg.found.data(), pg.found.size() * sizeof(int));
  return 0;
}

int *bnn_mi355x_read_page(const uint8_t *pixels, int width, int height, int bands, long row_stride, const bnn_mi355x_glyph_opts *opts,
                          const bnn_mi355x_find_opts *find, const bnn_mi355x_page_opts *page, int number_class, int cap, int *n_found, int *boxes,
                          int *line, int *gap, float *usecPerImage, float *usecPreprocess, int *status) {
  const PageOpts g = page_opts(page);
  return read_page("read_page", pixels, width, height, bands, row_stride, opts, find, &g, number_class, cap, n_found, boxes, line, gap, usecPerImage,
                   usecPreprocess, status);
}

int *bnn_mi355x_read_glyphs(const uint8_t *pixels, int width, int height, int bands, long row_stride, const bnn_mi355x_glyph_opts *opts,
                            const bnn_mi355x_find_opts *find, int number_class, int cap, int *n_found, int *boxes, float *usecPerImage,
                            float *usecPreprocess, int *status) {
  return read_page("read_glyphs", pixels, width, height, bands, row_stride, opts, find, nullptr, number_class, cap, n_found, boxes, nullptr, nullptr,
                   usecPerImage, usecPreprocess, status);
}

}  // extern "C"
