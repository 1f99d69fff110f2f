/* The similarity of the matcher's specification, stated on the host: sim[i][j] = the float32 fmaf chain over ascending k. */
#include <math.h>
#include <stdint.h>

void sim_fmaf(const float* a, const float* b, int64_t na, int64_t nb, int64_t dim, float* sim) {
  for (int64_t i = 0; i < na; ++i)
    for (int64_t j = 0; j < nb; ++j) {
      float s = 0.0f;
      for (int64_t k = 0; k < dim; ++k) s = fmaf(a[i * dim + k], b[j * dim + k], s);
      sim[i * nb + j] = s;
    }
}
