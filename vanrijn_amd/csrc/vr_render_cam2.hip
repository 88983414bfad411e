// vr_render_cam2.hip -- the render kernels of camera mode 2 (the scene's pose and lens): every instantiation
// launch_render_class<2> reaches (vr_render_kernel.h).
#include "vr_render_kernel.h"

namespace vr {
template hipError_t launch_render_class<2>(int, const RenderArgs&, const PoseArgs&, const LensArgs&, const LaunchChoice&,
                                           int, hipStream_t);
}  // namespace vr
