// The decomposition of a similarity Scw = [s*Rcw | s*tcw] that ORBmatcher::SearchByProjection(pKF, Scw, ...) (src/ORBmatcher.cc:298-303)
// and ORBmatcher::Fuse(pKF, Scw, ...) (:1142-1147) perform before they project: DESIGN.md Q41.  One statement, shared by the library
// (sd_api.hip) and the CPU oracle (tests/cpp/loop_oracle.cpp); plain C++, no device code.
//   scw = (float)sqrt(sum in f64 of the squares of row 0)       sqrt(sRcw.row(0).dot(sRcw.row(0))): cv::Mat::dot accumulates in double
//   inv = (float)(1.0 / (double)scw)                             how `Mat / scalar` is READ to evaluate: one reciprocal, then a multiply
//   Rcw = sRcw * inv, tcw = t * inv                              element-wise in f32
// That reading of OpenCV's `Mat / scalar` is not a checked fact (OpenCV is absent here): it is the frozen choice.
#pragma once
#include <cmath>

// Scw: row-major 4x4.  T: row-major 4x4 [Rcw | tcw; 0 0 0 1].
inline void sd_scw_decompose(const float* Scw, float* T)
{
    double ss = (double)Scw[0] * (double)Scw[0];
    ss += (double)Scw[1] * (double)Scw[1];
    ss += (double)Scw[2] * (double)Scw[2];
    const float scw = (float)std::sqrt(ss);
    const float inv = (float)(1.0 / (double)scw);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) T[4 * r + c] = Scw[4 * r + c] * inv;
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}
