// rome_conv_pose3.hip -- Pose3Pose3 (+ PriorPose3 rows) on the kernels of rome_conv.hpp; the policy: rome_conv_p3.hpp.
#include "rome_conv_p3.hpp"

namespace rome {

hipError_t launch_conv_pose3pose3(const ConvArgs& a, int solver, hipStream_t s) { return launch_solver<P3P3>(a, solver, s); }
hipError_t launch_deconv_pose3(int family, const DeconvArgs& a, hipStream_t s) {
  return family == kDeconvPose3Pose3 ? launch_deconv_t<P3P3>(a, s) : hipErrorInvalidValue;
}

}  // namespace rome
