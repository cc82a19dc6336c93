// The optional per-launch timing of the forward (bench.py): the records and the flm_profile_* calls are process state
// in flm_api.hip; the forward (flm_api_fcn.hip) brackets each launch with a ProfScope.  Host only.
#pragma once

#include "flm_common.h"

namespace flm {

struct ProfRec {
  const char* name;
  hipEvent_t a, b;
};
// The next free record with event `a` recorded on s, or null: profiling off, the records used up, a null name (the
// caller holds a record already) or a layer the filter leaves out.
ProfRec* prof_begin(hipStream_t s, const char* name);

struct ProfScope {
  hipStream_t s;
  ProfRec* r;
  ProfScope(hipStream_t st, const char* name) : s(st), r(prof_begin(st, name)) {}
  ~ProfScope() {
    if (r) (void)hipEventRecord(r->b, s);
  }
};

}  // namespace flm
