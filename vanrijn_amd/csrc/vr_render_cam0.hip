// vr_render_cam0.hip -- the render kernels of camera mode 0 (the default pose): every instantiation
// launch_render_class<0> reaches (vr_render_kernel.h).
#include "vr_render_kernel.h"

namespace vr {
template hipError_t launch_render_class<0>(int, const RenderArgs&, const PoseArgs&, const LensArgs&, const LaunchChoice&,
                                           int, hipStream_t);
}  // namespace vr
