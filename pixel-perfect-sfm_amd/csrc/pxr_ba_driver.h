// pxr_ba_driver.h -- host side of the BA driver, shared by pxr_ba_lists.hip (structure of a solve) and pxr_ba_solve.hip
// (buffers, LM loop): the solve's device buffers, its environment knobs, the structure stage.  Not part of the C-ABI.
#pragma once
#include <chrono>
#include <vector>

#include "pxr_ba_solve.h"

namespace pxr {


#define RC(call) do { int _rc = (call); if (_rc != PXR_OK) return _rc; } while (0)
#define LAUNCH_CHECK(name) RC(pxr::hip_check(hipGetLastError(), name))

// a work buffer of the running solve: from the context's arena when it has room, else from hipMalloc (solve_scratch)
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  bool owned = true;
  int alloc(size_t count) {
    n = count;
    p = static_cast<T*>(solve_scratch(sizeof(T) * (count ? count : 1), &owned));
    return p ? PXR_OK : set_error(PXR_ENOMEM, "hipMalloc(solver buffer): %zu bytes", sizeof(T) * count);
  }
  int upload(const std::vector<T>& h, hipStream_t s) {
    int rc = alloc(h.size());
    if (rc) return rc;
    if (!h.empty()) return hip_check(hipMemcpyAsync(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, s), "H2D");
    return PXR_OK;
  }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p && owned) (void)hipFree(p); }
};

// a StructError of pxr_ba_structure.h as the library's error (its formats take up to three %lld, nothing else)
inline int struct_error(const StructError& e) { return set_error(PXR_EINVAL, e.fmt, e.v[0], e.v[1], e.v[2]); }

// the environment knobs of a solve, read once per call (tests flip them between solves of one process)
struct SolveKnobs {
  bool arena, setup_host, verbose, spin_wait, inner_packed, inner_no_cache, inner_no_prebuild, schur_lds, phase_timing;
  SolveKnobs();
};

// PXR_VERBOSE: where the set-up's time goes
struct SetupClock {
  bool verbose;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void mark(const char* what) const {
    if (verbose)
      fprintf(stderr, "[pxr_ba_solve] setup: %-28s at %.2f ms\n", what,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
};

// pxr_ba_lists.hip: the structure of a solve -- block layout, observation lists per image and per point, the chunkings and the
// flattened index chains of the Schur / back-substitution kernels -- on the host and on the device
struct SolveStructure {
  // host
  std::vector<int32_t> image_camera, cam_model;
  BlockLayout layout;
  std::vector<int64_t> img_ptr;             // [n_images + 1] first slot of every image in the image-ordered list
  HostLists host;                           // host-built lists only (alive while their uploads may be in flight)
  std::vector<ImgChunk> chunks, schur_chunks;
  int64_t n_pvar = 0;                       // variable points
  bool device_lists = false;
  // device
  DevBuf<unsigned long long> d_cnt;
  DevBuf<int> d_flags;
  DevBuf<int> d_pose_off, d_pose_dim, d_tmask, d_intr_off, d_intr_dim, d_cmask, d_pt_var;
  DevBuf<ImgChunk> d_chunks, d_schur_chunks;
  DevBuf<uint8_t> d_pt_const;
  DevBuf<unsigned long long> d_pt_part;
  DevBuf<int64_t> d_img_obs, d_pt_ptr, d_pt_obs;
  DevBuf<int4> d_obs_cols, d_so;            // column descriptors in pt_obs order; {obs, point, first partner, partners} in img_obs order
  DevBuf<int> d_part_obs;
};
int build_structure(pxr_ctx* ctx, const pxr_ba_view* view, const uint8_t* h_pose_const, const uint8_t* h_tvec_const_mask,
                    const uint16_t* h_cam_const_mask, const uint8_t* h_point_const, const SolveKnobs& knobs, const SetupClock& clock,
                    SolveStructure* out);

}  // namespace pxr
