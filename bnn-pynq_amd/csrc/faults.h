// faults.h -- random bit/word-flip injection into the parameter memories.
//
// Mirrors the reference's fault campaign machinery (bnn/src/library/host/faults.h:30-148,
// topology.h:29-178, foldedmv-offload.h:146-214): faults land at uniformly distributed
// positions of the weight / threshold memories (selection weighted by the bit count of each
// layer) and at uniformly distributed image indices; a fault flips `word_size` adjacent bits
// of one memory word through the FoldedMVMemRead / FoldedMVMemSet path and stays in place.
// The reference seeds every generator from std::random_device; here the seed can be fixed
// (bnn_mi355x_set_fault_seed) so that a campaign can be replayed and checked.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "packed_params.h"
#include "topology.h"

namespace bnn {

struct Fault {
  int image;      // injected before this image is classified
  int target;     // 0 weights, 1 thresholds ("activations" in the reference's naming)
  int layer, mem, ind, thresh, bit, word_size;
};

// target_type: < 0 any, 0 weights, > 0 thresholds (main_python.cpp:105-108).  Returns "" and the plan, or the
// reason why the request cannot be honoured as asked (a target layer outside the network; thresholds-only
// faults on layers without threshold memory): never a silently different campaign.
std::string plan_faults(const NetSpec &net, uint64_t seed, int num_images, unsigned flip_count, int word_size,
                        int target_type, const int *target_layers, unsigned num_layers, std::vector<Fault> &out);

// inject_fault_impl on the raw memories; returns the matrix row whose packed form changed, or -1
int apply_fault(const NetSpec &net, RawParams &raw, const Fault &f);

// the raw word apply_fault(net, raw, f) modifies, or null where it would return -1.  apply_fault is not an involution
// (a layer-0 threshold is read back as its integer part): undoing a fault means restoring this word.
uint64_t *fault_word(const NetSpec &net, RawParams &raw, const Fault &f);

// Every distinct single fault of one layer's weight (target 0) or threshold (target 1) memory: the positions
// plan_faults can draw, the bit aligned down to a multiple of word_size as apply_fault aligns it, ordered by
// (mem, ind, thresh, bit).  Returns their number (0: a layer without threshold memory), -1 for a bad layer, target
// or word_size; writes faults first .. first + cap - 1 of them to out (image 0).
long enumerate_faults(const NetSpec &net, int layer, int target, int word_size, long first, Fault *out, long cap);

// "" when f lies inside the memories plan_faults draws from (the bit inside its element), else the reason
std::string check_fault(const NetSpec &net, const Fault &f);

}  // namespace bnn
