// The workspace layout of csrc/pxr_batch.h (Workspace) and the one grow of csrc/pxr_internal.h (grow_block) as host code over the
// stand-in runtime (on_host.h, hip/hip_runtime.h), on their own: no driver, no kernel.  emu_ws_layout lays a list of arrays out on
// a context, commits, reports where every pointer landed and writes every array from its first to its last byte;
// emu_ws_fail_once commits with the stand-in hipMalloc made to fail once and reports what became of the context's caches.  The
// expected offsets are computed by tests/test_workspace_lanes_cpu.py, not here.
// With -DWORKSPACE_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that runs the list given on its
// command line as kind:count words -- the list, the list again, its first half, the list with every count tripled -- and then
// the two failure cases, and prints what the exports report.  The block has exactly the layout's size, so a write past an
// array's end, or a pointer into a block that was freed, is caught.
#include "on_host.h"
#include "pxr_batch.h"

namespace {

struct Rec24 { double a; int32_t b[4]; };       // a 24-byte element
static_assert(sizeof(Rec24) == 24, "Rec24");

// one array of the list: `kind` says which member is taken (all are struct members; const and non-const pointees)
struct Array {
  uint8_t* u8; const uint8_t* cu8; int32_t* i32; const int32_t* ci32; double* f64; const double* cf64; Rec24* rec; const Rec24* crec;
};
constexpr int KINDS = 8;
constexpr size_t ELEM[KINDS] = {1, 1, 4, 4, 8, 8, 24, 24};

void take(pxr::Workspace& ws, Array& a, int kind, size_t count) {
  switch (kind) {
    case 0: ws.take(a.u8, count); break;
    case 1: ws.take(a.cu8, count); break;
    case 2: ws.take(a.i32, count); break;
    case 3: ws.take(a.ci32, count); break;
    case 4: ws.take(a.f64, count); break;
    case 5: ws.take(a.cf64, count); break;
    case 6: ws.take(a.rec, count); break;
    default: ws.take(a.crec, count); break;
  }
}
const void* taken(const Array& a, int kind) {
  const void* p[KINDS] = {a.u8, a.cu8, a.i32, a.ci32, a.f64, a.cf64, a.rec, a.crec};
  return p[kind];
}

}  // namespace

// n arrays of kinds[k] (see Array) and counts[k] elements, laid out on ctx and committed.  offsets[k]: where array k's pointer
// points, relative to the committed block (-1: the pointer was not filled).  info: {the block moved, hipMalloc calls of the
// commit, ctx->workspace_bytes afterwards}.
extern "C" int emu_ws_layout(pxr_ctx* ctx, int n, const int32_t* kinds, const int64_t* counts, int64_t* offsets, int64_t* info) {
  for (int k = 0; k < n; ++k)
    if (kinds[k] < 0 || kinds[k] >= KINDS || counts[k] < 0) return pxr::set_error(-1, "array %d: kind %d, count %lld", k, (int)kinds[k], (long long)counts[k]);
  const void* base_before = ctx->d_workspace;
  const int calls_before = emu_malloc_calls;
  static char unfilled;
  std::vector<Array> arrays((size_t)n);          // (sized before the first take: the layout remembers where the pointers live)
  for (Array& a : arrays) { a.u8 = (uint8_t*)&unfilled; a.cu8 = a.u8; a.i32 = (int32_t*)&unfilled; a.ci32 = a.i32; a.f64 = (double*)&unfilled; a.cf64 = a.f64; a.rec = (Rec24*)&unfilled; a.crec = a.rec; }
  pxr::Workspace ws;
  for (int k = 0; k < n; ++k) take(ws, arrays[(size_t)k], kinds[k], (size_t)counts[k]);
  if (int rc = ws.commit(ctx)) return rc;
  char* base = static_cast<char*>(ctx->d_workspace);
  for (int k = 0; k < n; ++k) {
    const char* p = static_cast<const char*>(taken(arrays[(size_t)k], kinds[k]));
    offsets[k] = p == &unfilled ? -1 : (int64_t)(p - base);
    if (p != &unfilled && counts[k] > 0) memset(const_cast<char*>(p), 0x5a, (size_t)counts[k] * ELEM[kinds[k]]);
  }
  info[0] = ctx->d_workspace != base_before;
  info[1] = emu_malloc_calls - calls_before;
  info[2] = (int64_t)ctx->workspace_bytes;
  return 0;
}

// One array of `bytes` bytes committed while the next hipMalloc fails, on a context that holds a Gram cache and a solve arena of
// 64 bytes each; `release`: whether the commit may release them.  out: {the commit's return code, d_gram is NULL, gram_bytes,
// d_solve_arena is NULL, solve_arena_bytes, workspace_bytes, hipMalloc calls of the commit, the pointer was filled}.
extern "C" int emu_ws_fail_once(pxr_ctx* ctx, int release, int64_t bytes, int64_t* out) {
  if (ctx->d_gram || ctx->d_solve_arena) return pxr::set_error(-1, "the context already holds a cache");
  ctx->d_gram = malloc(64); ctx->gram_bytes = 64;
  ctx->d_solve_arena = malloc(64); ctx->solve_arena_bytes = 64;
  const int calls_before = emu_malloc_calls;
  emu_malloc_failures = 1;
  uint8_t* p = nullptr;
  pxr::Workspace ws;
  ws.take(p, (size_t)bytes);
  out[0] = ws.commit(ctx, release != 0);
  emu_malloc_failures = 0;
  out[1] = ctx->d_gram == nullptr; out[2] = (int64_t)ctx->gram_bytes;
  out[3] = ctx->d_solve_arena == nullptr; out[4] = (int64_t)ctx->solve_arena_bytes;
  out[5] = (int64_t)ctx->workspace_bytes;
  out[6] = emu_malloc_calls - calls_before;
  out[7] = p != nullptr;
  if (p) memset(p, 0x5a, (size_t)bytes);
  free(ctx->d_gram); ctx->d_gram = nullptr; ctx->gram_bytes = 0;
  free(ctx->d_solve_arena); ctx->d_solve_arena = nullptr; ctx->solve_arena_bytes = 0;
  return 0;
}

#ifdef WORKSPACE_ON_HOST_MAIN
namespace {
int run(pxr_ctx* ctx, const char* name, const std::vector<int32_t>& kinds, const std::vector<int64_t>& counts) {
  std::vector<int64_t> offsets(kinds.size());
  int64_t info[3];
  if (int rc = emu_ws_layout(ctx, (int)kinds.size(), kinds.data(), counts.data(), offsets.data(), info)) { printf("%s failed %d: %s\n", name, rc, emu_last_error()); return rc; }
  printf("%s moved %lld mallocs %lld bytes %lld offsets", name, (long long)info[0], (long long)info[1], (long long)info[2]);
  for (int64_t o : offsets) printf(" %lld", (long long)o);
  printf("\n");
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  std::vector<int32_t> kinds;
  std::vector<int64_t> counts, tripled;
  for (int k = 1; k < argc; ++k) {
    int kind; long long count;
    if (sscanf(argv[k], "%d:%lld", &kind, &count) != 2) { printf("bad word %s\n", argv[k]); return 1; }
    kinds.push_back(kind); counts.push_back(count); tripled.push_back(3 * count);
  }
  pxr_ctx* ctx = emu_ctx();
  const size_t half = kinds.size() / 2;
  int rc = run(ctx, "first", kinds, counts);
  if (!rc) rc = run(ctx, "again", kinds, counts);
  if (!rc) rc = run(ctx, "half", std::vector<int32_t>(kinds.begin(), kinds.begin() + half), std::vector<int64_t>(counts.begin(), counts.begin() + half));
  if (!rc) rc = run(ctx, "tripled", kinds, tripled);
  for (int release = 1; release >= 0 && !rc; --release) {
    int64_t out[8];
    rc = emu_ws_fail_once(ctx, release, (int64_t)ctx->workspace_bytes + 1000, out);
    printf("release %d:", release);
    for (int64_t v : out) printf(" %lld", (long long)v);
    printf("\n");
  }
  emu_ctx_free(ctx);
  return rc;
}
#endif
