// mmf_mixed_plan (include/mmf_hip.h): the host-only plan of mmf_analyze_mixed -- per batch row its
// position in the compact text / image / both lists.  Plain C++ with no HIP and no handle, so it also
// compiles on its own under the host sanitizers (tools/mixed_plan_check.cpp).
#include <cstddef>
#include <cstdint>

#include "../../include/mmf_hip.h"

extern "C" int mmf_mixed_plan(const uint8_t* modality, int B, int32_t* row_map, int32_t* counts) {
  if (!modality || !row_map || !counts || B <= 0) return MMF_EINVAL;
  int32_t n[3] = {0, 0, 0};
  for (int b = 0; b < B; ++b) {
    const int m = modality[b];
    if (m < 1 || m > 3) return MMF_EINVAL;  // no modality (the reference's ValueError) or an unknown bit
    const bool in[3] = {(m & 1) != 0, (m & 2) != 0, m == 3};
    for (int l = 0; l < 3; ++l) row_map[(size_t)b * 3 + l] = in[l] ? n[l]++ : -1;
  }
  for (int l = 0; l < 3; ++l) counts[l] = n[l];
  return MMF_OK;
}
