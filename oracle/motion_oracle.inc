// TEST INFRASTRUCTURE — part of the CPU oracle (included by sd_oracle.cpp inside extern "C").
// The model fit of Tracking::TrackHomo (src/Tracking.cc:1026-1075): cv::findHomography(points_last, points_current,
// RANSAC, 3, inliers_H), cv::findFundamentalMat(points_last, points_current, RANSAC, 3, 0.99, inliers_F) and the
// choice `n_H > n_F ? (H, 1) : (F, 2)` when either has more than 10 inliers.
//
// OpenCV's two functions cannot be reproduced bit for bit without OpenCV (its RNG stream, 7-point solver, LM polish),
// so the algorithm is a SPEC of this build (DESIGN.md Q13), restated here independently of the device code:
//   * Hartley normalisation of both point sets exactly as Initializer::Normalize (src/Initializer.cc:749-795), in f64;
//   * up to 512 hypotheses for H (from 4 pairs) and 1024 for F (from 8 pairs) whose samples come from a counter-based
//     generator (splitmix64), so every hypothesis is independent of the others; like OpenCV's RANSAC the search stops
//     early when the best inlier ratio w makes further samples pointless, (1 - w^m)^k <= 1 - confidence, but the test is
//     made at one fixed checkpoint per model: after 64 H hypotheses (count >= 0.53 N, confidence 0.995) and after 128 F
//     hypotheses (count >= 0.66 N, confidence 0.99);
//   * H from 4 pairs: the 8x8 system with h33 = 1 (Gaussian elimination, partial pivoting); F from 8 pairs: rows of
//     Initializer::ComputeF21 (:305-343), null vector by elimination with complete pivoting, rank 2 by removing the
//     smallest right singular direction (3x3 cyclic Jacobi on F^T F);
//   * inliers as OpenCV counts them [OpenCV-recall]: H: |x2 - H x1|^2 <= 9; F: max(d1^2, d2^2) <= 9 with d = distance
//     to the epipolar line in each image, both evaluated in cross-multiplied form (no division); best = most inliers, the lowest hypothesis index on ties;
//   * H is then refitted on the best hypothesis' inliers by the normalised DLT of Initializer::ComputeH21 (:246-272;
//     smallest eigenvector of A^T A by 9x9 Jacobi, 15 sweeps in round-robin order: the four disjoint index pairs with
//     p + q = r (mod 9) are rotated together, r = 0..8) — no LM polish; the masks are those of the best hypotheses.
#define ORC_MOTION_KH 512
#define ORC_MOTION_KF 1024
#define ORC_MOTION_KH0 64
#define ORC_MOTION_KF0 128
#define ORC_MOTION_WH 0.53
#define ORC_MOTION_WF 0.66

static inline uint64_t orc_splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// draws `need` distinct indices below N for hypothesis h of model m; false when 64 draws do not suffice
static bool orc_motion_sample(int m, int h, int N, int need, int* idx)
{
    int got = 0;
    for (int c = 0; c < 64 && got < need; c++) {
        const int cand = (int)(orc_splitmix64(((uint64_t)(m * 4096 + h) << 6) + (uint64_t)c) % (uint64_t)N);
        bool dup = false;
        for (int j = 0; j < got; j++) dup |= idx[j] == cand;
        if (!dup) idx[got++] = cand;
    }
    return got == need;
}

struct OrcNorm { double meanX, meanY, sX, sY; bool ok; };
static OrcNorm orc_motion_normalize(const float* p, int N)      // p: N x 2
{
    OrcNorm n; n.ok = false; n.meanX = n.meanY = 0; n.sX = n.sY = 0;
    for (int i = 0; i < N; i++) { n.meanX += (double)p[2 * i]; n.meanY += (double)p[2 * i + 1]; }
    n.meanX = n.meanX / N; n.meanY = n.meanY / N;
    double dx = 0, dy = 0;
    for (int i = 0; i < N; i++) { dx += fabs((double)p[2 * i] - n.meanX); dy += fabs((double)p[2 * i + 1] - n.meanY); }
    dx = dx / N; dy = dy / N;
    if (!(dx > 0) || !(dy > 0)) return n;
    n.sX = 1.0 / dx; n.sY = 1.0 / dy; n.ok = true;
    return n;
}

// cyclic Jacobi on a symmetric n x n matrix (row-major, destroyed); V = eigenvectors in columns
static void orc_jacobi(double* a, double* v, int n, int sweeps)
{
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) v[i * n + j] = i == j ? 1.0 : 0.0;
    for (int s = 0; s < sweeps; s++)
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = a[p * n + q];
                if (fabs(apq) < 1e-300) continue;
                const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < n; k++) {
                    const double akp = a[k * n + p], akq = a[k * n + q];
                    a[k * n + p] = c * akp - sn * akq; a[k * n + q] = sn * akp + c * akq;
                }
                for (int k = 0; k < n; k++) {
                    const double apk = a[p * n + k], aqk = a[q * n + k];
                    a[p * n + k] = c * apk - sn * aqk; a[q * n + k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < n; k++) {
                    const double vkp = v[k * n + p], vkq = v[k * n + q];
                    v[k * n + p] = c * vkp - sn * vkq; v[k * n + q] = sn * vkp + c * vkq;
                }
            }
}

// Jacobi on a symmetric 9 x 9 matrix in round-robin order: round r rotates the index pairs (p, q), p < q, p + q = r (mod 9) --
// four disjoint pairs -- with angles taken from the matrix as it stands at the start of the round; all column updates of the
// round are applied before its row updates.
static void orc_jacobi9_round_robin(double* a, double* v, int sweeps)
{
    const int n = 9;
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) v[i * n + j] = i == j ? 1.0 : 0.0;
    for (int s = 0; s < sweeps; s++)
        for (int r = 0; r < n; r++) {
            int P[4], Q[4], cnt = 0;
            for (int p = 0; p < n; p++) { const int q = ((r - p) % n + n) % n; if (p < q) { P[cnt] = p; Q[cnt] = q; cnt++; } }
            double C[4], S[4];
            bool rot[4];
            for (int g = 0; g < 4; g++) {
                const int p = P[g], q = Q[g];
                const double apq = a[p * n + q];
                rot[g] = !(fabs(apq) < 1e-300);
                C[g] = 1.0; S[g] = 0.0;
                if (!rot[g]) continue;
                const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                C[g] = 1.0 / sqrt(t * t + 1.0); S[g] = t * C[g];
            }
            for (int g = 0; g < 4; g++) {
                if (!rot[g]) continue;
                const int p = P[g], q = Q[g];
                for (int k = 0; k < n; k++) {
                    const double akp = a[k * n + p], akq = a[k * n + q];
                    a[k * n + p] = C[g] * akp - S[g] * akq; a[k * n + q] = S[g] * akp + C[g] * akq;
                }
            }
            for (int g = 0; g < 4; g++) {
                if (!rot[g]) continue;
                const int p = P[g], q = Q[g];
                for (int k = 0; k < n; k++) {
                    const double apk = a[p * n + k], aqk = a[q * n + k];
                    a[p * n + k] = C[g] * apk - S[g] * aqk; a[q * n + k] = S[g] * apk + C[g] * aqk;
                }
                for (int k = 0; k < n; k++) {
                    const double vkp = v[k * n + p], vkq = v[k * n + q];
                    v[k * n + p] = C[g] * vkp - S[g] * vkq; v[k * n + q] = S[g] * vkp + C[g] * vkq;
                }
            }
        }
}

// H (row-major 3x3, H[8] scaled to 1) from 4 normalised pairs; false when the system is singular
static bool orc_h_from_4(const double* n1, const double* n2, const int* idx, double* Hn)
{
    double M[8][9];
    for (int k = 0; k < 4; k++) {
        const double x = n1[2 * idx[k]], y = n1[2 * idx[k] + 1], u = n2[2 * idx[k]], v = n2[2 * idx[k] + 1];
        double* r0 = M[2 * k]; double* r1 = M[2 * k + 1];
        r0[0] = x; r0[1] = y; r0[2] = 1; r0[3] = 0; r0[4] = 0; r0[5] = 0; r0[6] = -u * x; r0[7] = -u * y; r0[8] = u;
        r1[0] = 0; r1[1] = 0; r1[2] = 0; r1[3] = x; r1[4] = y; r1[5] = 1; r1[6] = -v * x; r1[7] = -v * y; r1[8] = v;
    }
    for (int c = 0; c < 8; c++) {
        int piv = c;
        for (int r = c + 1; r < 8; r++) if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
        if (fabs(M[piv][c]) < 1e-12) return false;
        if (piv != c) for (int k = 0; k < 9; k++) { const double t = M[c][k]; M[c][k] = M[piv][k]; M[piv][k] = t; }
        for (int r = c + 1; r < 8; r++) {
            const double f = M[r][c] / M[c][c];
            for (int k = c; k < 9; k++) M[r][k] -= f * M[c][k];
        }
    }
    for (int c = 7; c >= 0; c--) {
        double s = M[c][8];
        for (int k = c + 1; k < 8; k++) s -= M[c][k] * Hn[k];
        Hn[c] = s / M[c][c];
    }
    Hn[8] = 1.0;
    return true;
}

static void orc_mat3_mul(const double* A, const double* B, double* C)
{
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { double s = 0; for (int k = 0; k < 3; k++) s += A[3 * i + k] * B[3 * k + j]; C[3 * i + j] = s; }
}

// H = T2^-1 Hn T1, scaled to H[8] = 1
static void orc_h_denormalize(const double* Hn, const OrcNorm& a, const OrcNorm& b, double* H)
{
    const double T1[9] = {a.sX, 0, -a.meanX * a.sX, 0, a.sY, -a.meanY * a.sY, 0, 0, 1};
    const double T2inv[9] = {1.0 / b.sX, 0, b.meanX, 0, 1.0 / b.sY, b.meanY, 0, 0, 1};
    double t[9];
    orc_mat3_mul(Hn, T1, t);
    orc_mat3_mul(T2inv, t, H);
    if (fabs(H[8]) > 1e-300) { const double s = 1.0 / H[8]; for (int k = 0; k < 9; k++) H[k] *= s; }
}

static bool orc_f_from_8(const double* n1, const double* n2, const int* idx, double* Fn)
{
    double M[8][9];
    int col[9];
    for (int k = 0; k < 9; k++) col[k] = k;
    for (int k = 0; k < 8; k++) {
        const double u1 = n1[2 * idx[k]], v1 = n1[2 * idx[k] + 1], u2 = n2[2 * idx[k]], v2 = n2[2 * idx[k] + 1];
        double* r = M[k];
        r[0] = u2 * u1; r[1] = u2 * v1; r[2] = u2; r[3] = v2 * u1; r[4] = v2 * v1; r[5] = v2; r[6] = u1; r[7] = v1; r[8] = 1;
    }
    for (int c = 0; c < 8; c++) {                          // complete pivoting
        int pr = c, pc = c;
        double best = -1;
        for (int r = c; r < 8; r++) for (int k = c; k < 9; k++) if (fabs(M[r][k]) > best) { best = fabs(M[r][k]); pr = r; pc = k; }
        if (best < 1e-12) return false;
        if (pr != c) for (int k = 0; k < 9; k++) { const double t = M[c][k]; M[c][k] = M[pr][k]; M[pr][k] = t; }
        if (pc != c) { for (int r = 0; r < 8; r++) { const double t = M[r][c]; M[r][c] = M[r][pc]; M[r][pc] = t; } const int t = col[c]; col[c] = col[pc]; col[pc] = t; }
        for (int r = c + 1; r < 8; r++) {
            const double f = M[r][c] / M[c][c];
            for (int k = c; k < 9; k++) M[r][k] -= f * M[c][k];
        }
    }
    double x[9];
    x[8] = 1.0;
    for (int c = 7; c >= 0; c--) {
        double s = -M[c][8] * x[8];
        for (int k = c + 1; k < 8; k++) s -= M[c][k] * x[k];
        x[c] = s / M[c][c];
    }
    double f[9], nrm = 0;
    for (int k = 0; k < 9; k++) { f[col[k]] = x[k]; nrm += x[k] * x[k]; }
    nrm = 1.0 / sqrt(nrm);
    for (int k = 0; k < 9; k++) f[k] *= nrm;
    // rank 2: F - (F v) v^T with v the eigenvector of the smallest eigenvalue of F^T F
    double G[9], V[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { double s = 0; for (int k = 0; k < 3; k++) s += f[3 * k + i] * f[3 * k + j]; G[3 * i + j] = s; }
    orc_jacobi(G, V, 3, 10);
    int sm = 0;
    for (int k = 1; k < 3; k++) if (G[4 * k] < G[4 * sm]) sm = k;
    const double v[3] = {V[sm], V[3 + sm], V[6 + sm]};
    for (int i = 0; i < 3; i++) {
        const double fv = f[3 * i] * v[0] + f[3 * i + 1] * v[1] + f[3 * i + 2] * v[2];
        for (int j = 0; j < 3; j++) Fn[3 * i + j] = f[3 * i + j] - fv * v[j];
    }
    return true;
}

// F = T2^T Fn T1
static void orc_f_denormalize(const double* Fn, const OrcNorm& a, const OrcNorm& b, double* F)
{
    const double T1[9] = {a.sX, 0, -a.meanX * a.sX, 0, a.sY, -a.meanY * a.sY, 0, 0, 1};
    const double T2t[9] = {b.sX, 0, 0, 0, b.sY, 0, -b.meanX * b.sX, -b.meanY * b.sY, 1};
    double t[9];
    orc_mat3_mul(Fn, T1, t);
    orc_mat3_mul(T2t, t, F);
}

// The 3-px predicates in cross-multiplied form (no division: the same inequalities, |x2 - H x1|^2 <= 9 multiplied through by w^2,
// d^2 / (a^2 + b^2) <= 9 by the line's norm), each product and sum in the order written.
static inline bool orc_h_inlier(const double* H, double x1, double y1, double x2, double y2)
{
    const double w = H[6] * x1 + H[7] * y1 + H[8];
    const double A = H[0] * x1 + H[1] * y1 + H[2], B = H[3] * x1 + H[4] * y1 + H[5];
    const double dx = A - x2 * w, dy = B - y2 * w;
    return dx * dx + dy * dy <= 9.0 * (w * w);          // false for NaN
}
static inline bool orc_f_inlier(const double* F, double x1, double y1, double x2, double y2)
{
    double a = F[0] * x1 + F[1] * y1 + F[2], b = F[3] * x1 + F[4] * y1 + F[5], c = F[6] * x1 + F[7] * y1 + F[8];
    const double n2 = a * a + b * b, d2 = x2 * a + y2 * b + c;
    a = F[0] * x2 + F[3] * y2 + F[6]; b = F[1] * x2 + F[4] * y2 + F[7]; c = F[2] * x2 + F[5] * y2 + F[8];
    const double n1 = a * a + b * b, d1 = x1 * a + y1 * b + c;
    return d1 * d1 <= 9.0 * n1 && d2 * d2 <= 9.0 * n2;
}

// p1 = points_last, p2 = points_current (N x 2 f32).  Outputs: H, F (9 f64, zeros when not found), masks, counts,
// HorF (9 f32) and the return value of TrackHomo's choice: 1 (H), 2 (F) or 0.  info (6 ints or NULL) tells the tests which
// branches a point set reached: the winning hypothesis of H and of F (index inside its model, -1 = none), whether the search
// of H / of F stopped at its checkpoint (1) or ran the full hypothesis set (0), and how many of the hypotheses it looked at
// were degenerate (the sampler found no 4 / 8 distinct pairs, or the minimal system was singular) for H / for F.
int orc_estimate_motion_ex(const float* p1, const float* p2, int N, double* Hout, double* Fout, uint8_t* maskH, uint8_t* maskF,
                           int* nH, int* nF, float* HorF, int* info /*[6]: bestH bestF stopH stopF degH degF*/)
{
    int stopH = 0, stopF = 0, degH = 0, degF = 0;
    if (info) { info[0] = -1; info[1] = -1; for (int k = 2; k < 6; k++) info[k] = 0; }
    for (int k = 0; k < 9; k++) { Hout[k] = 0; Fout[k] = 0; HorF[k] = 0; }
    for (int i = 0; i < N; i++) { maskH[i] = 0; maskF[i] = 0; }
    *nH = 0; *nF = 0;
    if (N < 8) return 0;
    const OrcNorm a = orc_motion_normalize(p1, N), b = orc_motion_normalize(p2, N);
    if (!a.ok || !b.ok) return 0;
    std::vector<double> n1(2 * N), n2(2 * N);
    for (int i = 0; i < N; i++) {
        n1[2 * i] = ((double)p1[2 * i] - a.meanX) * a.sX; n1[2 * i + 1] = ((double)p1[2 * i + 1] - a.meanY) * a.sY;
        n2[2 * i] = ((double)p2[2 * i] - b.meanX) * b.sX; n2[2 * i + 1] = ((double)p2[2 * i + 1] - b.meanY) * b.sY;
    }
    // ---- homography
    int bestH = -1, bestHn = 0;
    double Hbest[9] = {0};
    for (int h = 0; h < ORC_MOTION_KH; h++) {
        if (h == ORC_MOTION_KH0 && (double)bestHn >= ORC_MOTION_WH * (double)N) { stopH = 1; break; }        // the checkpoint test
        int idx[4];
        double Hn[9], H[9];
        if (!orc_motion_sample(0, h, N, 4, idx) || !orc_h_from_4(n1.data(), n2.data(), idx, Hn)) { degH++; continue; }
        orc_h_denormalize(Hn, a, b, H);
        int cnt = 0;
        for (int i = 0; i < N; i++) cnt += orc_h_inlier(H, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]);
        if (cnt > bestHn) { bestHn = cnt; bestH = h; memcpy(Hbest, H, sizeof(H)); }
    }
    if (bestH >= 0 && bestHn >= 4) {
        for (int i = 0; i < N; i++) maskH[i] = orc_h_inlier(Hbest, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]);
        *nH = bestHn;
        // refit: Initializer::ComputeH21 on the inliers (normalised), A^T A accumulated row by row
        double M[81];
        for (int k = 0; k < 81; k++) M[k] = 0;
        for (int i = 0; i < N; i++) {
            if (!maskH[i]) continue;
            const double u1 = n1[2 * i], v1 = n1[2 * i + 1], u2 = n2[2 * i], v2 = n2[2 * i + 1];
            const double r0[9] = {0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2};
            const double r1[9] = {u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2};
            for (int p = 0; p < 9; p++) for (int q = 0; q < 9; q++) { M[9 * p + q] += r0[p] * r0[q]; M[9 * p + q] += r1[p] * r1[q]; }
        }
        double V[81];
        orc_jacobi9_round_robin(M, V, 15);
        int sm = 0;
        for (int k = 1; k < 9; k++) if (M[10 * k] < M[10 * sm]) sm = k;
        double Hn[9];
        for (int k = 0; k < 9; k++) Hn[k] = V[9 * k + sm];
        orc_h_denormalize(Hn, a, b, Hout);
    }
    // ---- fundamental matrix
    int bestF = -1, bestFn = 0;
    double Fbest[9] = {0};
    for (int h = 0; h < ORC_MOTION_KF; h++) {
        if (h == ORC_MOTION_KF0 && (double)bestFn >= ORC_MOTION_WF * (double)N) { stopF = 1; break; }
        int idx[8];
        double Fn[9], F[9];
        if (!orc_motion_sample(1, h, N, 8, idx) || !orc_f_from_8(n1.data(), n2.data(), idx, Fn)) { degF++; continue; }
        orc_f_denormalize(Fn, a, b, F);
        int cnt = 0;
        for (int i = 0; i < N; i++) cnt += orc_f_inlier(F, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]);
        if (cnt > bestFn) { bestFn = cnt; bestF = h; memcpy(Fbest, F, sizeof(F)); }
    }
    if (bestF >= 0 && bestFn >= 8) {
        for (int i = 0; i < N; i++) maskF[i] = orc_f_inlier(Fbest, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]);
        *nF = bestFn;
        memcpy(Fout, Fbest, sizeof(Fbest));
    }
    if (info) { info[0] = bestH; info[1] = bestF; info[2] = stopH; info[3] = stopF; info[4] = degH; info[5] = degF; }
    // ---- Tracking.cc:1060-1072
    if (*nF > 10 || *nH > 10) {
        if (*nH > *nF) { for (int k = 0; k < 9; k++) HorF[k] = (float)Hout[k]; return 1; }
        for (int k = 0; k < 9; k++) HorF[k] = (float)Fout[k];
        return 2;
    }
    return 0;
}

int orc_estimate_motion(const float* p1, const float* p2, int N, double* Hout, double* Fout, uint8_t* maskH, uint8_t* maskF,
                        int* nH, int* nF, float* HorF)
{
    return orc_estimate_motion_ex(p1, p2, N, Hout, Fout, maskH, maskF, nH, nF, HorF, nullptr);
}
