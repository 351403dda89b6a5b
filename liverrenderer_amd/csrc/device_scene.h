// Interface between the plain-C++ part of the library (capi.cpp) and the HIP
// translation unit (device.hip).  All functions throw std::runtime_error.
#pragma once
#include "../../include/liverrt.h"
#include <initializer_list>
#include <vector>

namespace lrt {
struct DeviceScene;
DeviceScene *device_scene_create(const lrt_scene_desc &d, int device);
void device_scene_destroy(DeviceScene *d);
void device_scene_update_params(DeviceScene *D, const lrt_scene_desc &d, bool grids = false);   // grids: the heterogeneous media's grid values changed too
void device_render(DeviceScene *D, const lrt_scene_desc &d, const lrt_render_opts *opts, float *film_raw, float *image, lrt_render_stats &stats);
void device_develop(DeviceScene *D, const float *film_raw, float *image, int on_device);
// the aov integrator (kernels_aov.h): nested renders, then the first-hit AOV pass; merged image on the device
void device_render_aov(DeviceScene *D, const lrt_scene_desc &d, const lrt_aov_desc &aov, const lrt_render_opts *opts, float *aov_film_raw, float *image, lrt_render_stats &stats);
void device_render_aov_samples(DeviceScene *D, const lrt_scene_desc &d, const lrt_aov_desc &aov, const lrt_render_opts *opts, uint64_t lane_begin, uint32_t n, float *out, lrt_render_stats &stats);
// the moment integrator (kernels_moment.h): the nested integrator's lanes, then the moment film (R,G,B,[A],W,X,Y,Z,m2X,m2Y,m2Z)
void device_render_moment(DeviceScene *D, const lrt_scene_desc &d, const lrt_render_opts *opts, float *film_raw, float *image, lrt_render_stats &stats);
void device_render_moment_samples(DeviceScene *D, const lrt_scene_desc &d, const lrt_render_opts *opts, uint64_t lane_begin, uint32_t n, float *out, lrt_render_stats &stats);
void device_render_samples(DeviceScene *D, const lrt_scene_desc &d, const lrt_render_opts *opts, uint64_t lane_begin, uint32_t n, float *out, lrt_render_stats &stats);
void device_trace(DeviceScene *D, const lrt_rays_soa *rays, const lrt_hits_soa *hits, uint32_t n, int any_hit);
// the per-pixel primary entry the device image holds, as the host built it (scene_prep.h: build_primary_entry); empty: the image has no table
const std::vector<uint16_t> &device_primary_entry(const DeviceScene *D);
// test hooks (probes.h): one piece of the shading code per lane.  The kinds are named here because capi.cpp names them and cannot see device code.
enum ProbeKind { PROBE_EMITTER, PROBE_ENVMAP, PROBE_BSDF, PROBE_PHASE, PROBE_MEDIUM, PROBE_SENSOR, PROBE_KINDS };
struct ProbeColumn { const float *p; int width; };   // one input array of a probe call: `width` floats per lane
void device_probe(DeviceScene *D, ProbeKind kind, int arg, std::initializer_list<ProbeColumn> columns, uint32_t n, float *out);
// network stage of the learned subsurface model (kernels_vae.h): host arrays in, host arrays out
void device_vae_scatter(const float *blob, uint32_t n, const float *in_pos, const float *in_dir, const float *poly, const float albedo[3], float g, float ior,
                        const float sigma_t[3], float fit_scale, uint32_t seed, float *out_pos, float *out_absorption, int device);
void device_render_backward(DeviceScene *D, const lrt_scene_desc &d, const lrt_render_opts *opts, const float *grad_image, lrt_param_grads *out, lrt_render_stats &stats,
                            float *d_grid = nullptr);   // d_grid: lrt_render_backward_grid (host or device pointer, as opts->output_on_device says)
void device_math_eval(int fn, const float *x, const float *y, uint32_t n, float *out, float *out2, int device);   // test hook: dmath.h on the device
// guided denoiser (kernels_denoise.h): the workspace and a non-blocking stream belong to the object; `params` arrives resolved (no zeros)
struct Denoiser;
Denoiser *denoiser_create(int width, int height, bool use_albedo, bool use_normals, bool denoise_alpha, const lrt_denoise_params &params, int device);
void denoiser_destroy(Denoiser *d);
void denoiser_run(Denoiser *d, const float *noisy, int channels, const float *albedo, const float *normals, float *out, int device_buffers);
// one process, several devices: tiles over the devices, one RCCL all-reduce of the film / of the 7 gradient doubles (device.hip)
struct MultiContext;
void multi_context_destroy(MultiContext *m);
void device_render_multi(std::vector<DeviceScene *> &devs, MultiContext *&ctx, const lrt_scene_desc &d, const lrt_render_opts *opts, float *film_raw, float *image, lrt_render_stats &stats);
void device_render_backward_multi(std::vector<DeviceScene *> &devs, MultiContext *&ctx, const lrt_scene_desc &d, const lrt_render_opts *opts, const float *grad_image, lrt_param_grads *out, lrt_render_stats &stats);
} // namespace lrt
