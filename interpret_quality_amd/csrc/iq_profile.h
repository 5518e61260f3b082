// RAII HIP-event bracket around a kernel launch, recorded on the launch stream (bench.py's
// roofline leg reads the totals through iq_profile_read).  Costs nothing when disabled.
#pragma once
#include <hip/hip_runtime.h>

namespace iq {

// kSlotDominant: the ONE kernel that dominates a model's step (bench.py's per-model roofline), with the FLOP its MFMA tiles
// execute attached as `work`
enum ProfileSlot { kSlotPrepool = 0, kSlotFstn = 1, kSlotTrunk = 2, kSlotCall = 3, kSlotMask = 4, kSlotDominant = 5 };

bool profile_enabled();

class ProfileSpan {
  public:
    ProfileSpan(int which, hipStream_t st, double work = 0.0);
    ~ProfileSpan();
    ProfileSpan(const ProfileSpan&) = delete;
    ProfileSpan& operator=(const ProfileSpan&) = delete;

  private:
    int which_;
    hipStream_t st_;
    bool on_;
    double work_;
    hipEvent_t start_{}, stop_{};
};

}  // namespace iq
