// What the launchers of the pair walk share (compare.hip defines them;
// sort.hip uses them): the plan's class table on the device and the LDS
// threshold of the walk.
#pragma once
#include "host_common.h"

namespace xdrg {
namespace host {

struct cmp_tables {
  const uint32_t *d_info;
  const cmp_word *d_prog;
};

constexpr size_t kCmpLdsOps = 48u << 10;  // plans whose ops and classes fit are walked from LDS

// XDRG_EUNSUPPORTED for a plan with U32 / U64 / UNION ops and no classes;
// a plan with nothing to classify gets all-zero classes.  Host only.
int cmp_classes_ready(const xdrg_plan *plan);
// The class table and the word program on the current device: uploaded
// (synchronously, one allocation) by the plan's first compare or sort there.
int cmp_upload(const xdrg_plan *plan, cmp_tables *out);

}  // namespace host
}  // namespace xdrg
