// Device half of page_to_mnist / read_page (see page.h): the masked twin of the glyph record kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glyph_kernels.h"
#include "page.h"

namespace bnn {

// Record i at records + i * 784 (16-byte aligned) from desc[i], keys[2 i ..] and the tables in coef, as
// launch_glyph_record -- but a pixel of the plane counts only where the label plane holds one of the glyph's two key
// values, and is 255 elsewhere.  label: width x height ints, index y * width + x, as launch_cc_collect leaves it
// (component_kernels.h): a component's root pixel holds -2 - id, its other pixels its first pixel, background -1.
// Every desc's ink box lies inside the picture (the caller has checked the component list).
hipError_t launch_page_record(const GlyphPicture &p, const int32_t *label, const GlyphDesc *desc, const int32_t *keys, const int32_t *coef,
                              uint8_t *tmp, uint8_t *records, int n, hipStream_t s);

}  // namespace bnn
