// pxr_ba_structure.h -- the host-side structure of a BA solve: everything the LM driver computes on the host from index arrays
// and constancy masks.  Plain C++ without a HIP header, so that it builds (and runs under a sanitizer) without a GPU:
// tests/host/ba_structure_main.cpp.  Not part of the C-ABI.
//
// Functions return 0 or fill a StructError: a printf format whose only conversions are up to three %lld (the caller hands it
// to set_error with all three values: struct_error, pxr_ba_driver.h).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#ifdef __HIP__   // (the attributes spelt out: no HIP header is included here)
#define PXR_STRUCT_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define PXR_STRUCT_HD inline
#endif

namespace pxr {

// [upstream COLMAP 3.8 camera_models.h] number of parameters by model id
constexpr int kNumCameraModels = 11;
constexpr int kNumParams[kNumCameraModels] = {3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12};

struct ImgChunk { int img; int64_t begin, end; };   // observations [begin, end) of the image-ordered slot list
struct alignas(8) IntPair { int x, y; };            // the layout of HIP's int2 (checked where the tables reach the kernels)

struct StructError { const char* fmt = nullptr; long long v[3] = {0, 0, 0}; };
inline int struct_fail(StructError* e, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
  e->fmt = fmt; e->v[0] = a; e->v[1] = b; e->v[2] = c;
  return 1;
}

// global column index of camera-side column `a` of an observation in image img / camera cam: the pose columns of the image, then
// the variable intrinsics of its camera.  THE rule, for the kernels (col_index, pxr_ba_solve.h) and for the tables below.
PXR_STRUCT_HD int column_of(const int* pose_off, const int* pose_dim, const int* intr_off, int img, int cam, int a) {
  const int pd = pose_dim[img];
  return a < pd ? pose_off[img] + a : intr_off[cam] + (a - pd);
}

// ---- block layout: which camera-side blocks are in the program and where their columns are ------------------------------------
// With several ranks a camera-side block may have no local observation but still be part of the (global) program: the caller
// marks unused blocks constant, every non-constant block is kept.
struct BlockLayout {
  std::vector<int> pose_off, pose_dim, tmask;   // per image
  std::vector<int> intr_off, intr_dim, cmask;   // per camera
  int n_c = 0;                                  // reduced system size
  int DC = 1;                                   // max camera-side columns of an observation
  int LS = 13;                                  // stride of the linearisation record: 11 + 2 DC
  int dc(int img, int cam) const { return pose_dim[img] + intr_dim[cam]; }
  int column(int img, int cam, int a) const { return column_of(pose_off.data(), pose_dim.data(), intr_off.data(), img, cam, a); }
};
inline int block_layout(int n_img, int n_cam, const uint8_t* pose_const, const uint8_t* tvec_const_mask, const uint16_t* cam_const_mask,
                        const int32_t* cam_model, BlockLayout* out, StructError* err) {
  for (int c = 0; c < n_cam; ++c)
    if (cam_model[c] < 0 || cam_model[c] >= kNumCameraModels) return struct_fail(err, "pxr_ba_solve: unsupported camera model id %lld", cam_model[c]);
  BlockLayout& l = *out;
  l.pose_off.resize(n_img); l.pose_dim.resize(n_img); l.tmask.resize(n_img);
  l.intr_off.resize(n_cam); l.intr_dim.resize(n_cam); l.cmask.resize(n_cam);
  int off = 0, dpose_max = 0, dintr_max = 0;
  for (int i = 0; i < n_img; ++i) {
    int d = 0;
    l.tmask[i] = tvec_const_mask[i] & 7;
    if (!pose_const[i]) d = 3 + (3 - __builtin_popcount(l.tmask[i]));
    l.pose_off[i] = off; l.pose_dim[i] = d; off += d;
    dpose_max = std::max(dpose_max, d);
  }
  for (int c = 0; c < n_cam; ++c) {
    const int K = kNumParams[cam_model[c]];
    l.cmask[c] = cam_const_mask[c] & ((1 << K) - 1);
    const int d = K - __builtin_popcount(l.cmask[c]);
    l.intr_off[c] = off; l.intr_dim[c] = d; off += d;
    dintr_max = std::max(dintr_max, d);
  }
  l.n_c = off;
  l.DC = std::max(1, dpose_max + dintr_max);
  l.LS = 11 + 2 * l.DC;
  return 0;
}

inline int require_variable_block(int n_c, int64_t n_pvar, StructError* err) {
  return (n_c > 0 || n_pvar > 0) ? 0 : struct_fail(err, "pxr_ba_solve: every parameter block is constant");
}

// ---- chunks of the image-ordered slot list: one workgroup each (512 slots for k_img, 1024 for the Schur contraction) ------------
inline std::vector<ImgChunk> chunk_images(const std::vector<int64_t>& img_ptr, int64_t per_chunk) {
  std::vector<ImgChunk> chunks;
  for (int i = 0; i + 1 < (int)img_ptr.size(); ++i)
    for (int64_t b = img_ptr[i]; b < img_ptr[i + 1]; b += per_chunk) chunks.push_back({i, b, std::min(img_ptr[i + 1], b + per_chunk)});
  return chunks;
}
// where an image's chunks start (chunks are image-major)
inline std::vector<int> first_chunks(const std::vector<ImgChunk>& chunks, int n_img) {
  std::vector<int> ptr(n_img + 1, 0);
  for (const ImgChunk& c : chunks) ++ptr[c.img + 1];
  for (int i = 0; i < n_img; ++i) ptr[i + 1] += ptr[i];
  return ptr;
}

// ---- observation lists per image and per point, built on the host (the general path: input not ordered by point, more images
// than the device sort takes, PXR_BA_SETUP_HOST=1) -- ascending observation id inside an image / a point ---------------------------
struct HostLists {
  std::vector<int64_t> img_ptr, pt_ptr;   // prefix sums of the counts
  std::vector<int64_t> img_obs, pt_obs;   // observation ids, image-ordered / point-ordered
  std::vector<int> pt_var;                // the point is not constant and has an observation
  int64_t n_pvar = 0;
};
inline int host_lists(int64_t n_obs, const int32_t* obs_image, const int32_t* obs_point, int n_img, int64_t n_pts,
                      const uint8_t* point_const, int n_c, HostLists* out, StructError* err) {
  HostLists& h = *out;
  h.img_ptr.assign(n_img + 1, 0); h.pt_ptr.assign(n_pts + 1, 0);
  for (int64_t i = 0; i < n_obs; ++i) {
    if (!(obs_image[i] >= 0 && obs_image[i] < n_img && obs_point[i] >= 0 && obs_point[i] < n_pts))
      return struct_fail(err, "pxr_ba_solve: observation %lld references image %lld / point %lld out of range", i, obs_image[i], obs_point[i]);
    ++h.img_ptr[obs_image[i] + 1]; ++h.pt_ptr[obs_point[i] + 1];
  }
  h.pt_var.resize(n_pts);
  h.n_pvar = 0;
  for (int64_t p = 0; p < n_pts; ++p) { h.pt_var[p] = (!point_const[p] && h.pt_ptr[p + 1] > 0) ? 1 : 0; h.n_pvar += h.pt_var[p]; }
  if (require_variable_block(n_c, h.n_pvar, err)) return 1;
  for (int64_t p = 0; p < n_pts; ++p) h.pt_ptr[p + 1] += h.pt_ptr[p];
  for (int i = 0; i < n_img; ++i) h.img_ptr[i + 1] += h.img_ptr[i];
  h.img_obs.resize(n_obs); h.pt_obs.resize(n_obs);
  std::vector<int64_t> ic(h.img_ptr.begin(), h.img_ptr.end() - 1), pc(h.pt_ptr.begin(), h.pt_ptr.end() - 1);
  for (int64_t i = 0; i < n_obs; ++i) { h.img_obs[ic[obs_image[i]]++] = i; h.pt_obs[pc[obs_point[i]]++] = i; }
  return 0;
}

// ---- preconditioner blocks of the iterative solver: the pose columns of an image and the intrinsics columns of a camera; one
// joint block where the camera belongs to a single image (every column in exactly one block).  group_cols: [n_groups][gs] ---------
struct PrecondBlocks {
  std::vector<IntPair> col_group;         // per column: {block, row inside it}
  std::vector<int> group_size, group_cols;
};
inline int precond_blocks(const BlockLayout& l, const int32_t* image_camera, int gs, PrecondBlocks* out, StructError* err) {
  const int n_img = (int)l.pose_dim.size(), n_cam = (int)l.intr_dim.size();
  if (l.DC > gs) return struct_fail(err, "pxr_ba_solve: %lld camera-side columns per observation exceed the preconditioner block size", l.DC);
  PrecondBlocks& b = *out;
  std::vector<int> cam_users(n_cam, 0);
  for (int i = 0; i < n_img; ++i) ++cam_users[image_camera[i]];
  b.col_group.assign(l.n_c, IntPair{-1, -1});
  b.group_size.clear(); b.group_cols.clear();
  auto open_group = [&b, gs]() { b.group_size.push_back(0); b.group_cols.resize(b.group_cols.size() + gs, 0); return (int)b.group_size.size() - 1; };
  auto add_cols = [&b, gs](int g, int first, int count) {
    for (int a = 0; a < count; ++a) {
      b.col_group[first + a] = IntPair{g, b.group_size[g]};
      b.group_cols[(size_t)g * gs + b.group_size[g]++] = first + a;
    }
  };
  for (int i = 0; i < n_img; ++i) {
    const int c = image_camera[i];
    const bool joint = cam_users[c] == 1 && l.intr_dim[c] > 0;
    if (l.pose_dim[i] == 0 && !joint) continue;
    const int g = open_group();
    add_cols(g, l.pose_off[i], l.pose_dim[i]);
    if (joint) add_cols(g, l.intr_off[c], l.intr_dim[c]);
  }
  for (int c = 0; c < n_cam; ++c)
    if (cam_users[c] != 1 && l.intr_dim[c] > 0) add_cols(open_group(), l.intr_off[c], l.intr_dim[c]);
  for (int c = 0; c < l.n_c; ++c)
    if (b.col_group[c].x < 0) return struct_fail(err, "pxr_ba_solve: internal: column %lld in no preconditioner block", c);
  return 0;
}

// ---- deterministic mode of the iterative solver: the (image, local column) entries of every reduced-system column, images
// ascending -- the order of every column's sum ------------------------------------------------------------------------------------
struct ColumnEntries { std::vector<int> ent_ptr; std::vector<IntPair> ent; };
inline void column_entries(const BlockLayout& l, const int32_t* image_camera, ColumnEntries* out) {
  const int n_img = (int)l.pose_dim.size();
  std::vector<int>& ent_ptr = out->ent_ptr;
  ent_ptr.assign(l.n_c + 1, 0);
  for (int i = 0; i < n_img; ++i)
    for (int a = 0; a < l.dc(i, image_camera[i]); ++a) ++ent_ptr[l.column(i, image_camera[i], a) + 1];
  for (int c = 0; c < l.n_c; ++c) ent_ptr[c + 1] += ent_ptr[c];
  out->ent.resize(ent_ptr[l.n_c]);
  std::vector<int> fill(ent_ptr.begin(), ent_ptr.end() - 1);
  for (int i = 0; i < n_img; ++i)
    for (int a = 0; a < l.dc(i, image_camera[i]); ++a) out->ent[fill[l.column(i, image_camera[i], a)]++] = IntPair{i, a};
}

}  // namespace pxr
