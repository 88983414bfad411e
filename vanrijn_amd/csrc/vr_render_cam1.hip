// vr_render_cam1.hip -- the render kernels of camera mode 1 (the scene's pose): every instantiation
// launch_render_class<1> reaches (vr_render_kernel.h).
#include "vr_render_kernel.h"

namespace vr {
template hipError_t launch_render_class<1>(int, const RenderArgs&, const PoseArgs&, const LensArgs&, const LaunchChoice&,
                                           int, hipStream_t);
}  // namespace vr
