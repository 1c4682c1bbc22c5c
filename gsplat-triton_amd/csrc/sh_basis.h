// Real spherical-harmonics basis (degree 0..4) and its partials, shared by the
// SH colour kernels (sh.hip) and the appearance MLP (appearance.hip).
#pragma once

#include "common.h"

namespace gs {

// Basis values B[k] and partials dB[k] = (dB/dx, dB/dy, dB/dz) w.r.t. the
// normalised direction (sh_fwd.py:43-66 constants).
template <int DEG, bool GRAD>
GS_INLINE void sh_basis(float x, float y, float z, float *B, float (*dB)[3]) {
  B[0] = 0.28209479177387814f;
  if (GRAD) dB[0][0] = dB[0][1] = dB[0][2] = 0.f;
  if (DEG < 1) return;
  const float C1 = 0.4886025119029199f;
  B[1] = -C1 * y;
  B[2] = C1 * z;
  B[3] = -C1 * x;
  if (GRAD) {
    dB[1][0] = 0.f; dB[1][1] = -C1; dB[1][2] = 0.f;
    dB[2][0] = 0.f; dB[2][1] = 0.f; dB[2][2] = C1;
    dB[3][0] = -C1; dB[3][1] = 0.f; dB[3][2] = 0.f;
  }
  if (DEG < 2) return;
  const float zz = z * z;
  const float g2 = 2.f * x * y, h2 = x * x - y * y;
  const float C22 = 0.5462742152960396f;
  const float c21 = -1.0925484305920792f * z;
  B[4] = C22 * g2;
  B[5] = c21 * y;
  B[6] = 0.9461746957575601f * zz - 0.3153915652525201f;
  B[7] = c21 * x;
  B[8] = C22 * h2;
  if (GRAD) {
    dB[4][0] = 2.f * C22 * y; dB[4][1] = 2.f * C22 * x; dB[4][2] = 0.f;
    dB[5][0] = 0.f; dB[5][1] = c21; dB[5][2] = -1.0925484305920792f * y;
    dB[6][0] = 0.f; dB[6][1] = 0.f; dB[6][2] = 1.8923493915151202f * z;
    dB[7][0] = c21; dB[7][1] = 0.f; dB[7][2] = -1.0925484305920792f * x;
    dB[8][0] = 2.f * C22 * x; dB[8][1] = -2.f * C22 * y; dB[8][2] = 0.f;
  }
  if (DEG < 3) return;
  const float g3 = x * g2 + y * h2, h3 = x * h2 - y * g2;
  const float C33 = -0.5900435899266435f, C32 = 1.445305721320277f;
  const float c31 = -2.285228997322329f * zz + 0.4570457994644658f;
  B[9] = C33 * g3;
  B[10] = C32 * g2 * z;
  B[11] = c31 * y;
  B[12] = z * (1.865881662950577f * zz - 1.119528997770346f);
  B[13] = c31 * x;
  B[14] = C32 * h2 * z;
  B[15] = C33 * h3;
  if (GRAD) {
    const float dc31 = -4.570457994644658f * z;
    dB[9][0] = 3.f * C33 * g2; dB[9][1] = 3.f * C33 * h2; dB[9][2] = 0.f;
    dB[10][0] = 2.f * C32 * y * z; dB[10][1] = 2.f * C32 * x * z; dB[10][2] = C32 * g2;
    dB[11][0] = 0.f; dB[11][1] = c31; dB[11][2] = dc31 * y;
    dB[12][0] = 0.f; dB[12][1] = 0.f; dB[12][2] = 5.597644988851731f * zz - 1.119528997770346f;
    dB[13][0] = c31; dB[13][1] = 0.f; dB[13][2] = dc31 * x;
    dB[14][0] = 2.f * C32 * x * z; dB[14][1] = -2.f * C32 * y * z; dB[14][2] = C32 * h2;
    dB[15][0] = 3.f * C33 * h2; dB[15][1] = -3.f * C33 * g2; dB[15][2] = 0.f;
  }
  if (DEG < 4) return;
  const float g4 = x * g3 + y * h3, h4 = x * h3 - y * g3;
  const float C44 = 0.6258357354491761f, C43 = -1.7701307697799304f;
  const float c41 = z * (-4.683325804901024f * zz + 2.0071396306718676f);
  const float c42 = 3.31161143515146f * zz - 0.47308734787878f;
  B[16] = C44 * g4;
  B[17] = C43 * g3 * z;
  B[18] = c42 * g2;
  B[19] = c41 * y;
  B[20] = zz * (3.7024941420321507f * zz - 3.1735664074561294f) + 0.31735664074561293f;
  B[21] = c41 * x;
  B[22] = c42 * h2;
  B[23] = C43 * h3 * z;
  B[24] = C44 * h4;
  if (GRAD) {
    const float dc41 = -14.049977414703072f * zz + 2.0071396306718676f;
    const float dc42 = 6.62322287030292f * z;
    dB[16][0] = 4.f * C44 * g3; dB[16][1] = 4.f * C44 * h3; dB[16][2] = 0.f;
    dB[17][0] = 3.f * C43 * g2 * z; dB[17][1] = 3.f * C43 * h2 * z; dB[17][2] = C43 * g3;
    dB[18][0] = 2.f * c42 * y; dB[18][1] = 2.f * c42 * x; dB[18][2] = dc42 * g2;
    dB[19][0] = 0.f; dB[19][1] = c41; dB[19][2] = dc41 * y;
    dB[20][0] = 0.f; dB[20][1] = 0.f; dB[20][2] = z * (14.809976568128603f * zz - 6.347132814912259f);
    dB[21][0] = c41; dB[21][1] = 0.f; dB[21][2] = dc41 * x;
    dB[22][0] = 2.f * c42 * x; dB[22][1] = -2.f * c42 * y; dB[22][2] = dc42 * h2;
    dB[23][0] = 3.f * C43 * h2 * z; dB[23][1] = -3.f * C43 * g2 * z; dB[23][2] = C43 * h3;
    dB[24][0] = 4.f * C44 * h3; dB[24][1] = -4.f * C44 * g3; dB[24][2] = 0.f;
  }
}

}  // namespace gs
