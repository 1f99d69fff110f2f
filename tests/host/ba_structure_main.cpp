// Stand-alone driver of csrc/pxr_ba_structure.h (the host-side structure of a BA solve) for tests/test_ba_structure_cpu.py:
// reads a tiny problem from stdin, prints every table as one JSON object.  Built with -fsanitize=address,undefined and run as a
// program -- the header needs no GPU and no HIP.
//
// stdin (whitespace-separated integers): n_img n_cam n_pts n_obs, then image_camera[n_img] cam_model[n_cam] pose_const[n_img]
// tvec_const_mask[n_img] cam_const_mask[n_cam] point_const[n_pts] obs_image[n_obs] obs_point[n_obs]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pxr_ba_structure.h"

using namespace pxr;

template <typename T>
static std::vector<T> read(size_t n) {
  std::vector<T> v(n);
  for (auto& x : v) { long long t = 0; if (scanf("%lld", &t) != 1) { fprintf(stderr, "short input\n"); exit(2); } x = (T)t; }
  return v;
}
template <typename T>
static void put(const char* name, const std::vector<T>& v, const char* end = ",") {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? ", " : "", (long long)v[i]);
  printf("]%s\n", end);
}
static void put(const char* name, const std::vector<IntPair>& v) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s[%d, %d]", i ? ", " : "", v[i].x, v[i].y);
  printf("],\n");
}
static void put(const char* name, const std::vector<ImgChunk>& v) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s[%d, %lld, %lld]", i ? ", " : "", v[i].img, (long long)v[i].begin, (long long)v[i].end);
  printf("],\n");
}
static int fail(const StructError& e) {
  char msg[256];
  snprintf(msg, sizeof msg, e.fmt, e.v[0], e.v[1], e.v[2]);
  printf("\"error\": \"%s\"}\n", msg);
  return 0;
}

int main() {
  const std::vector<long long> dims = read<long long>(4);
  const int n_img = (int)dims[0], n_cam = (int)dims[1];
  const int64_t n_pts = dims[2], n_obs = dims[3];
  const auto image_camera = read<int32_t>(n_img), cam_model = read<int32_t>(n_cam);
  const auto pose_const = read<uint8_t>(n_img), tvec_mask = read<uint8_t>(n_img);
  const auto cam_mask = read<uint16_t>(n_cam);
  const auto point_const = read<uint8_t>(n_pts);
  const auto obs_image = read<int32_t>(n_obs), obs_point = read<int32_t>(n_obs);
  StructError err;
  printf("{");
  BlockLayout l;
  if (block_layout(n_img, n_cam, pose_const.data(), tvec_mask.data(), cam_mask.data(), cam_model.data(), &l, &err)) return fail(err);
  put("pose_off", l.pose_off); put("pose_dim", l.pose_dim); put("tmask", l.tmask);
  put("intr_off", l.intr_off); put("intr_dim", l.intr_dim); put("cmask", l.cmask);
  printf("\"n_c\": %d, \"DC\": %d, \"LS\": %d,\n", l.n_c, l.DC, l.LS);
  HostLists h;
  if (host_lists(n_obs, obs_image.data(), obs_point.data(), n_img, n_pts, point_const.data(), l.n_c, &h, &err)) return fail(err);
  put("img_ptr", h.img_ptr); put("pt_ptr", h.pt_ptr); put("img_obs", h.img_obs); put("pt_obs", h.pt_obs); put("pt_var", h.pt_var);
  printf("\"n_pvar\": %lld,\n", (long long)h.n_pvar);
  const std::vector<ImgChunk> c512 = chunk_images(h.img_ptr, 512), c1024 = chunk_images(h.img_ptr, 1024);
  put("chunks512", c512); put("chunks1024", c1024);
  put("first512", first_chunks(c512, n_img)); put("first1024", first_chunks(c1024, n_img));
  PrecondBlocks b;
  if (precond_blocks(l, image_camera.data(), 18, &b, &err)) return fail(err);
  put("col_group", b.col_group); put("group_size", b.group_size); put("group_cols", b.group_cols);
  ColumnEntries ce;
  column_entries(l, image_camera.data(), &ce);
  put("ent", ce.ent);
  put("ent_ptr", ce.ent_ptr, "}");
  return 0;
}
