// act_faults.h -- single faults in the inter-layer activation stream (bnn_mi355x_act_fault_sweep).
//
// A site is one activation of layer L's output as layer L+1 reads it (CNV layers 1 and 3: after the max-pool), for
// every layer but the last.  The fault replaces the activation's level index i (1-bit: -1, +1; 2-bit: -1, 0, +1) by
// (i + shift) mod levels, 1 <= shift < levels: a sign flip, or the next / the one after next of the three levels.
// The reference holds no activation-fault model (its TargetType::Activations means threshold memories): this one
// is the project's own.
#pragma once
#include <string>

#include "topology.h"

namespace bnn {

struct ActSite { int layer, y, x, channel, shift; };

// layer L's output map as the next layer reads it: h x w pixels of c channels, `levels` values per activation
struct ActShape { int h, w, c, levels; };

// false for the last layer (scores / words, no activations) or a layer out of range
bool act_shape(const NetSpec &net, int layer, ActShape *s);

// every site x shift of layer L ordered by (y, x, channel, shift); returns their number, -1 for a layer without
// sites; writes sites first .. first + cap - 1 to out
long enumerate_act_faults(const NetSpec &net, int layer, long first, ActSite *out, long cap);

// "" when the record names a site and a shift of a layer that has them, else the reason
std::string check_act_fault(const NetSpec &net, const ActSite &s);

}  // namespace bnn
