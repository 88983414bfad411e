// vr_render_launch.hip -- the render launch (host side): argument checks, the stack class, the camera mode's
// launcher, then the ordered reduce.  The render kernel and its launchers are vr_render_kernel.h; each
// camera mode's instantiations are compiled in a unit of their own (vr_render_cam0.hip, vr_render_cam1.hip,
// vr_render_cam2.hip), so the kernels build in parallel and this unit holds none.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/vanrijn_amd.h"
#include "vr_layout.h"

namespace vr {

// vr_render_kernel.h, instantiated by the camera units: enqueues the render kernel of the launch
template <int CAM>
hipError_t launch_render_class(int depth, const RenderArgs& a, const PoseArgs& pose, const LensArgs& lens,
                               const LaunchChoice& c, int grid_limit, hipStream_t s);
extern template hipError_t launch_render_class<0>(int, const RenderArgs&, const PoseArgs&, const LensArgs&,
                                                  const LaunchChoice&, int, hipStream_t);
extern template hipError_t launch_render_class<1>(int, const RenderArgs&, const PoseArgs&, const LensArgs&,
                                                  const LaunchChoice&, int, hipStream_t);
extern template hipError_t launch_render_class<2>(int, const RenderArgs&, const PoseArgs&, const LensArgs&,
                                                  const LaunchChoice&, int, hipStream_t);
// vr_reduce.hip: the render kernel's launch status, the `mid` event, then the ordered reduce
hipError_t launch_reduce(const RenderArgs& a, hipStream_t s, hipEvent_t mid);

int launch_render(const RenderArgs& a, const PoseArgs& pose, const LensArgs& lens, const LaunchChoice& c, int grid_limit,
                  void* stream, void* mid_event) {
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t mid = (hipEvent_t)mid_event;
    if (a.tile_width == 0 || a.tile_height == 0 || a.spp == 0) return 0;
    hipError_t e;
    // the 64-bit-offset kernels exist in the deepest stack class only (a scene that needs them is
    // far larger than any whose tree fits the smaller classes; more LDS is only fewer waves)
    const int depth = c.big && c.stack_depth <= 48 ? 48 : c.stack_depth;
    if (depth > 48) return -1000;
    // RenderArgs::posed: the instantiations whose camera step applies the scene's pose, or pose and lens
    if (a.posed == 2) e = launch_render_class<2>(depth, a, pose, lens, c, grid_limit, s);
    else if (a.posed) e = launch_render_class<1>(depth, a, pose, lens, c, grid_limit, s);
    else e = launch_render_class<0>(depth, a, pose, lens, c, grid_limit, s);
    // (hipErrorInvalidValue: no kernel of that class was launched, and there is nothing to reduce)
    if (e == hipSuccess) e = launch_reduce(a, s, mid);
    return (int)e;
}

const char* device_error_string(int code) {
    if (code == -1000) return "BVH deeper than the largest traversal stack (48)";
    return hipGetErrorString((hipError_t)code);
}

}  // namespace vr
