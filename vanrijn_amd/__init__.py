"""vanrijn_amd -- MI355X (gfx950) native core for vanrijn's per-pixel path-tracing hot path.

The product is the C-ABI library vanrijn_amd/lib/libvanrijn_amd.so (HIP kernels + C++ host,
include/vanrijn_amd.h).  This package is the host-side mirror of the reference's API over that
library; every pixel is computed on the GPU.
"""
from .render import (AccumulationBuffer, Film, ImageRgbU8, Tile, TileIterator, partial_render_scene, render_samples,
                     render_tile, render_tile_device, resolve_state, tone_map_device, trace_rays, RAY_HIT_DTYPE,
                     query_any, query_any_device, query_closest, query_closest_device, PHOTON_DTYPE,
                     PATH_INFO_DTYPE, integrate_rays, integrate_rays_device, accumulate_photons_device,
                     camera_rays_device, FeatureBuffers, render_features, render_features_device, DenoiseParams,
                     denoise, denoise_device, denoise_workspace_bytes, ReprojectParams, reproject, reproject_device,
                     motion_rows)
from .scene import (BoundingVolumeHierarchy, ColourRgbF, DeviceScene, DirectionalLight, LambertianMaterial,
                    MaterialSpec, Mesh, PrimitiveSpec, CameraPose, look_at, CameraLens, lens_point,
                    NamedColour, PhongMaterial, Plane, WhittedIntegrator, ReflectiveMaterial, Scene, SceneSpec, SmoothTransparentDialectric, Sphere,
                    Spectrum, load_obj, load_obj_groups)
from . import _native

__all__ = [
    "AccumulationBuffer", "Film", "ImageRgbU8", "Tile", "TileIterator", "partial_render_scene", "render_samples", "render_tile",
    "render_tile_device", "resolve_state", "tone_map_device", "trace_rays", "BoundingVolumeHierarchy", "ColourRgbF", "DeviceScene",
    "LambertianMaterial", "Mesh", "NamedColour", "PhongMaterial", "Plane", "ReflectiveMaterial", "Scene", "SceneSpec",
    "SmoothTransparentDialectric", "Sphere", "Spectrum", "load_obj", "DirectionalLight", "WhittedIntegrator",
    "RAY_HIT_DTYPE", "query_any", "query_any_device", "query_closest", "query_closest_device",
    "PHOTON_DTYPE", "PATH_INFO_DTYPE", "integrate_rays", "integrate_rays_device", "accumulate_photons_device",
    "camera_rays_device", "MaterialSpec", "PrimitiveSpec", "CameraPose", "look_at", "CameraLens", "lens_point",
    "load_obj_groups", "FeatureBuffers", "render_features", "render_features_device", "DenoiseParams", "denoise",
    "denoise_device", "denoise_workspace_bytes", "ReprojectParams", "reproject", "reproject_device", "motion_rows",
]


def device_count():
    return _native.lib().vr_device_count()
