// Stand-alone CPU check of csrc/stage_layout.h: for every null / non-null combination of the arguments of the
// host/device twin pairs, the total size and the offset of every sub-array against the sums altro_batch.hip wrote out by hand
// before the layout was shared, and the name, the required flag and the extent the `_dev` form validates against the sizes
// include/altro_batch.h documents.  No GPU, no library:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/stage_layout_check \
//       tools/stage_layout_check.cpp && /tmp/stage_layout_check
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../altro-mpc-icra2021_amd/csrc/stage_layout.h"

using altro::StageLayout;
static long checks = 0;

static void expect(bool ok, const char* what, int combo) {
  ++checks;
  if (ok) return;
  std::fprintf(stderr, "FAILED: %s (combination %d)\n", what, combo);
  std::exit(1);
}

// slot i: offset, room, whether the kernels get it, and that a sub-array handed to them is aligned for its type
static void slot_is(const StageLayout& L, int i, size_t off, size_t bytes, bool dev, size_t align, const char* what, int combo) {
  const StageLayout::Slot& s = L.slot[i];
  expect(s.bytes == bytes, what, combo);
  expect(bytes == 0 || s.off == off, what, combo);
  expect(s.dev == dev, what, combo);
  expect(!dev || s.off % align == 0, what, combo);
}

// slot i as the `_dev` form sees it: the argument's name, whether null is refused, and the bytes validated (present or not)
static void arg_is(const StageLayout& L, int i, const char* name, bool required, size_t extent, const char* what, int combo) {
  const StageLayout::Slot& s = L.slot[i];
  expect(s.name && std::strcmp(s.name, name) == 0, what, combo);
  expect(s.required == required, what, combo);
  expect(s.extent == extent, what, combo);
}

int main() {
  static double d[1];    // stands for a caller's array: only null / non-null matters here
  static int32_t i32[1];
  const size_t D = sizeof(double), I = sizeof(int32_t);
  const size_t dims[][5] = {{5, 9, 12, 4, 1}, {5, 9, 12, 4, 17}, {2, 4, 64, 32, 3}, {1, 2, 1, 1, 1}, {8192, 50, 12, 4, 8}};
  for (const auto& q : dims) {
    const size_t B = q[0], N = q[1], n = q[2], m = q[3], nc = q[4];
    // altro_batch_eval_policy: bytes = B (n + m) doubles + 2 B ints either way; x, u, knot, fb; x and u are required
    for (int c = 0; c < 4; ++c) {
      const int32_t* kn = c & 1 ? i32 : nullptr;
      int32_t* fb = c & 2 ? i32 : nullptr;
      StageLayout L;
      altro::stage_eval_policy(L, B, n, m, d, kn, d, fb);
      expect(L.nslots == 4, "eval_policy: slots", c);
      expect(L.bytes == B * (n + m) * D + 2 * B * I, "eval_policy: size", c);
      slot_is(L, altro::EP_X, 0, B * n * D, true, D, "eval_policy: x", c);
      slot_is(L, altro::EP_U, B * n * D, B * m * D, true, D, "eval_policy: u", c);
      slot_is(L, altro::EP_KNOT, B * (n + m) * D, B * I, kn, I, "eval_policy: knot", c);
      slot_is(L, altro::EP_FB, B * (n + m) * D + B * I, B * I, fb, I, "eval_policy: fb", c);
      expect(L.slot[altro::EP_X].in == d && L.slot[altro::EP_KNOT].in == kn && L.slot[altro::EP_U].out == d && L.slot[altro::EP_FB].out == fb &&
                 !L.slot[altro::EP_X].out && !L.slot[altro::EP_U].in && !L.slot[altro::EP_KNOT].out && !L.slot[altro::EP_FB].in,
             "eval_policy: copies", c);
      arg_is(L, altro::EP_X, "x", true, B * n * D, "eval_policy: arg x", c);
      arg_is(L, altro::EP_U, "u", true, B * m * D, "eval_policy: arg u", c);
      arg_is(L, altro::EP_KNOT, "knot", false, B * I, "eval_policy: arg knot", c);
      arg_is(L, altro::EP_FB, "fb", false, B * I, "eval_policy: arg fb", c);
    }
    // altro_batch_evaluate: elems = 3 R + (U ? cu : 0) + (X ? cx : 0) + (x0 ? B n : 0) + (Xout ? cx : 0); J, c_max, defect first
    for (int c = 0; c < 128; ++c) {
      const double *U = c & 1 ? d : nullptr, *X = c & 2 ? d : nullptr, *x0 = c & 4 ? d : nullptr;
      double *J = c & 8 ? d : nullptr, *cm = c & 16 ? d : nullptr, *df = c & 32 ? d : nullptr, *Xo = c & 64 ? d : nullptr;
      const size_t R = B * nc, cu = R * (N - 1) * m, cx = R * N * n;
      StageLayout L;
      altro::stage_evaluate(L, B, N, n, m, nc, U, X, x0, J, cm, df, Xo);
      expect(L.nslots == 7, "evaluate: slots", c);
      expect(L.bytes == (3 * R + (U ? cu : 0) + (X ? cx : 0) + (x0 ? B * n : 0) + (Xo ? cx : 0)) * D, "evaluate: size", c);
      size_t s = 0;
      slot_is(L, altro::EV_J, s, R * D, J, D, "evaluate: J", c); s += R * D;
      slot_is(L, altro::EV_CMAX, s, R * D, cm, D, "evaluate: c_max", c); s += R * D;
      slot_is(L, altro::EV_DEFECT, s, R * D, df, D, "evaluate: defect", c); s += R * D;
      slot_is(L, altro::EV_U, s, U ? cu * D : 0, U, D, "evaluate: U", c); s += U ? cu * D : 0;
      slot_is(L, altro::EV_X, s, X ? cx * D : 0, X, D, "evaluate: X", c); s += X ? cx * D : 0;
      slot_is(L, altro::EV_X0, s, x0 ? B * n * D : 0, x0, D, "evaluate: x0", c); s += x0 ? B * n * D : 0;
      slot_is(L, altro::EV_XOUT, s, Xo ? cx * D : 0, Xo, D, "evaluate: Xout", c);
      expect((L.slot[altro::EV_U].in == U) && (L.slot[altro::EV_J].out == J) && (L.slot[altro::EV_XOUT].out == Xo), "evaluate: copies", c);
      arg_is(L, altro::EV_U, "U", false, B * nc * (N - 1) * m * D, "evaluate: arg U", c);
      arg_is(L, altro::EV_X, "X", false, B * nc * N * n * D, "evaluate: arg X", c);
      arg_is(L, altro::EV_X0, "x0", false, B * n * D, "evaluate: arg x0", c);
      arg_is(L, altro::EV_J, "J", false, B * nc * D, "evaluate: arg J", c);
      arg_is(L, altro::EV_CMAX, "c_max", false, B * nc * D, "evaluate: arg c_max", c);
      arg_is(L, altro::EV_DEFECT, "defect", false, B * nc * D, "evaluate: arg defect", c);
      arg_is(L, altro::EV_XOUT, "Xout", false, B * nc * N * n * D, "evaluate: arg Xout", c);
    }
    // altro_batch_evaluate_grad: elems = 2 R + (gU ? cu : 0) + (gx0 ? R n : 0) + (U ? cu : 0) + (x0 ? B n : 0) + (Xout ? cx : 0); J, P first
    for (int c = 0; c < 128; ++c) {
      const double *U = c & 1 ? d : nullptr, *x0 = c & 2 ? d : nullptr;
      double *J = c & 4 ? d : nullptr, *P = c & 8 ? d : nullptr, *gU = c & 16 ? d : nullptr, *g0 = c & 32 ? d : nullptr, *Xo = c & 64 ? d : nullptr;
      const size_t R = B * nc, cu = R * (N - 1) * m, cx = R * N * n;
      StageLayout L;
      altro::stage_evaluate_grad(L, B, N, n, m, nc, U, x0, J, P, gU, g0, Xo);
      expect(L.nslots == 7, "evaluate_grad: slots", c);
      size_t s = 0;
      slot_is(L, altro::EG_J, s, R * D, J, D, "evaluate_grad: J", c); s += R * D;
      slot_is(L, altro::EG_P, s, R * D, P, D, "evaluate_grad: P", c); s += R * D;
      slot_is(L, altro::EG_GU, s, gU ? cu * D : 0, gU, D, "evaluate_grad: gU", c); s += gU ? cu * D : 0;
      slot_is(L, altro::EG_GX0, s, g0 ? R * n * D : 0, g0, D, "evaluate_grad: gx0", c); s += g0 ? R * n * D : 0;
      slot_is(L, altro::EG_U, s, U ? cu * D : 0, U, D, "evaluate_grad: U", c); s += U ? cu * D : 0;
      slot_is(L, altro::EG_X0, s, x0 ? B * n * D : 0, x0, D, "evaluate_grad: x0", c); s += x0 ? B * n * D : 0;
      slot_is(L, altro::EG_XOUT, s, Xo ? cx * D : 0, Xo, D, "evaluate_grad: Xout", c); s += Xo ? cx * D : 0;
      expect(L.bytes == s, "evaluate_grad: size", c);
      expect(L.slot[altro::EG_U].in == U && L.slot[altro::EG_X0].in == x0 && L.slot[altro::EG_GU].out == gU && L.slot[altro::EG_XOUT].out == Xo,
             "evaluate_grad: copies", c);
      arg_is(L, altro::EG_U, "U", true, B * nc * (N - 1) * m * D, "evaluate_grad: arg U", c);
      arg_is(L, altro::EG_X0, "x0", false, B * n * D, "evaluate_grad: arg x0", c);
      arg_is(L, altro::EG_J, "J", false, B * nc * D, "evaluate_grad: arg J", c);
      arg_is(L, altro::EG_P, "P", false, B * nc * D, "evaluate_grad: arg P", c);
      arg_is(L, altro::EG_GU, "gU", false, B * nc * (N - 1) * m * D, "evaluate_grad: arg gU", c);
      arg_is(L, altro::EG_GX0, "gx0", false, B * nc * n * D, "evaluate_grad: arg gx0", c);
      arg_is(L, altro::EG_XOUT, "Xout", false, B * nc * N * n * D, "evaluate_grad: arg Xout", c);
    }
    // altro_batch_evaluate_al: every one of the fourteen sub-arrays only when given, the twelve outputs of altro_al_out in the
    // order of the struct, then U, then x0
    for (int c = 0; c < (1 << 14); ++c) {
      const size_t R = B * nc, cu = R * (N - 1) * m, cx = R * N * n;
      const size_t cnt[14] = {R, R, cu, R * n, cx, cu, R * n, R * n, R * m, R * (n + m), R * (n + m), cx, cu, B * n};
      double* out[12];
      for (int i = 0; i < 12; ++i) out[i] = (c >> i) & 1 ? d : nullptr;
      const double *U = (c >> 12) & 1 ? d : nullptr, *x0 = (c >> 13) & 1 ? d : nullptr;
      StageLayout L;
      altro::stage_evaluate_al(L, B, N, n, m, nc, U, x0, out);
      expect(L.nslots == altro::AL_SLOTS && L.nslots <= StageLayout::MAX_SLOTS, "evaluate_al: slots", c);
      size_t s = 0;
      for (int i = 0; i < 14; ++i) {
        const bool on = (c >> i) & 1;
        slot_is(L, i, s, on ? cnt[i] * D : 0, on, D, "evaluate_al: sub-array", c);
        s += on ? cnt[i] * D : 0;
        expect(L.slot[i].out == (i < 12 ? out[i] : nullptr) && L.slot[i].in == (i == 12 ? U : i == 13 ? x0 : nullptr), "evaluate_al: copies", c);
      }
      expect(L.bytes == s, "evaluate_al: size", c);
      arg_is(L, altro::AL_LA, "LA", false, B * nc * D, "evaluate_al: arg LA", c);
      arg_is(L, altro::AL_J, "J", false, B * nc * D, "evaluate_al: arg J", c);
      arg_is(L, altro::AL_GU, "gU", false, B * nc * (N - 1) * m * D, "evaluate_al: arg gU", c);
      arg_is(L, altro::AL_GX0, "gx0", false, B * nc * n * D, "evaluate_al: arg gx0", c);
      arg_is(L, altro::AL_GXREF, "gXref", false, B * nc * N * n * D, "evaluate_al: arg gXref", c);
      arg_is(L, altro::AL_GUREF, "gUref", false, B * nc * (N - 1) * m * D, "evaluate_al: arg gUref", c);
      arg_is(L, altro::AL_GQ, "gQ", false, B * nc * n * D, "evaluate_al: arg gQ", c);
      arg_is(L, altro::AL_GQF, "gQf", false, B * nc * n * D, "evaluate_al: arg gQf", c);
      arg_is(L, altro::AL_GR, "gR", false, B * nc * m * D, "evaluate_al: arg gR", c);
      arg_is(L, altro::AL_GZMIN, "gzmin", false, B * nc * (n + m) * D, "evaluate_al: arg gzmin", c);
      arg_is(L, altro::AL_GZMAX, "gzmax", false, B * nc * (n + m) * D, "evaluate_al: arg gzmax", c);
      arg_is(L, altro::AL_XOUT, "Xout", false, B * nc * N * n * D, "evaluate_al: arg Xout", c);
      arg_is(L, altro::AL_U, "U", false, B * nc * (N - 1) * m * D, "evaluate_al: arg U", c);
      arg_is(L, altro::AL_X0, "x0", false, B * n * D, "evaluate_al: arg x0", c);
      expect(altro::AL_LA == 0 && altro::AL_XOUT == 11 && altro::AL_U == 12 && altro::AL_X0 == 13, "evaluate_al: order", c);
    }
    // altro_batch_warm_start: bytes = (2 R1 + cu) doubles + B ints; J, c_max, U, chosen, all handed to the kernels
    for (int c = 0; c < 16; ++c) {
      const size_t inc = c & 1;
      int32_t* ch = c & 2 ? i32 : nullptr;
      double *J = c & 4 ? d : nullptr, *cm = c & 8 ? d : nullptr;
      const size_t R1 = B * (nc + inc), cu = B * nc * (N - 1) * m;
      StageLayout L;
      altro::stage_warm_start(L, B, N, m, nc, inc, d, ch, J, cm);
      expect(L.nslots == 4, "warm_start: slots", c);
      expect(L.bytes == (2 * R1 + cu) * D + B * I, "warm_start: size", c);
      slot_is(L, altro::WS_J, 0, R1 * D, true, D, "warm_start: J", c);
      slot_is(L, altro::WS_CMAX, R1 * D, R1 * D, true, D, "warm_start: c_max", c);
      slot_is(L, altro::WS_U, 2 * R1 * D, cu * D, true, D, "warm_start: U", c);
      slot_is(L, altro::WS_CHOSEN, (2 * R1 + cu) * D, B * I, true, I, "warm_start: chosen", c);
      expect(L.slot[altro::WS_U].in == d && L.slot[altro::WS_CHOSEN].out == ch && L.slot[altro::WS_J].out == J, "warm_start: copies", c);
      arg_is(L, altro::WS_U, "U", true, B * nc * (N - 1) * m * D, "warm_start: arg U", c);
      arg_is(L, altro::WS_CHOSEN, "chosen", false, B * I, "warm_start: arg chosen", c);
      arg_is(L, altro::WS_J, "J", false, B * (nc + inc) * D, "warm_start: arg J", c);
      arg_is(L, altro::WS_CMAX, "c_max", false, B * (nc + inc) * D, "warm_start: arg c_max", c);
    }
    // altro_batch_simulate_policy: elems = 3 R + (x0 ? c0 : 0) + (w ? cw : 0) + (Xout ? cx : 0) + (Uout ? cu : 0) doubles + B ints
    for (int c = 0; c < 256; ++c) {
      const double *x0 = c & 1 ? d : nullptr, *w = c & 2 ? d : nullptr;
      double *J = c & 4 ? d : nullptr, *cm = c & 8 ? d : nullptr, *dx = c & 16 ? d : nullptr, *Xo = c & 64 ? d : nullptr, *Uo = c & 128 ? d : nullptr;
      int32_t* fb = c & 32 ? i32 : nullptr;
      const size_t R = B * nc, c0 = R * n, cw = R * (N - 1) * n, cx = R * N * n, cu = R * (N - 1) * m;
      StageLayout L;
      altro::stage_simulate(L, B, N, n, m, nc, x0, w, J, cm, dx, fb, Xo, Uo);
      expect(L.nslots == 8, "simulate: slots", c);
      expect(L.bytes == (3 * R + (x0 ? c0 : 0) + (w ? cw : 0) + (Xo ? cx : 0) + (Uo ? cu : 0)) * D + B * I, "simulate: size", c);
      size_t s = 0;
      slot_is(L, altro::SIM_J, s, R * D, J, D, "simulate: J", c); s += R * D;
      slot_is(L, altro::SIM_CMAX, s, R * D, cm, D, "simulate: c_max", c); s += R * D;
      slot_is(L, altro::SIM_DXMAX, s, R * D, dx, D, "simulate: dx_max", c); s += R * D;
      slot_is(L, altro::SIM_X0, s, x0 ? c0 * D : 0, x0, D, "simulate: x0", c); s += x0 ? c0 * D : 0;
      slot_is(L, altro::SIM_W, s, w ? cw * D : 0, w, D, "simulate: w", c); s += w ? cw * D : 0;
      slot_is(L, altro::SIM_XOUT, s, Xo ? cx * D : 0, Xo, D, "simulate: Xout", c); s += Xo ? cx * D : 0;
      slot_is(L, altro::SIM_UOUT, s, Uo ? cu * D : 0, Uo, D, "simulate: Uout", c); s += Uo ? cu * D : 0;
      slot_is(L, altro::SIM_FB, s, B * I, fb, I, "simulate: fb", c);
      expect(L.slot[altro::SIM_X0].in == x0 && L.slot[altro::SIM_W].in == w && L.slot[altro::SIM_FB].out == fb, "simulate: copies", c);
      arg_is(L, altro::SIM_X0, "x0", false, B * nc * n * D, "simulate: arg x0", c);
      arg_is(L, altro::SIM_W, "w", false, B * nc * (N - 1) * n * D, "simulate: arg w", c);
      arg_is(L, altro::SIM_J, "J", false, B * nc * D, "simulate: arg J", c);
      arg_is(L, altro::SIM_CMAX, "c_max", false, B * nc * D, "simulate: arg c_max", c);
      arg_is(L, altro::SIM_DXMAX, "dx_max", false, B * nc * D, "simulate: arg dx_max", c);
      arg_is(L, altro::SIM_FB, "fb", false, B * I, "simulate: arg fb", c);
      arg_is(L, altro::SIM_XOUT, "Xout", false, B * nc * N * n * D, "simulate: arg Xout", c);
      arg_is(L, altro::SIM_UOUT, "Uout", false, B * nc * (N - 1) * m * D, "simulate: arg Uout", c);
    }
    // altro_batch_propagate_covariance: dJ and fb have room either way, the eight others only when given; fb last (ints)
    for (int c = 0; c < 2048; ++c) {
      const double *S0 = c & 1 ? d : nullptr, *W = c & 2 ? d : nullptr;
      double *sx = c & 4 ? d : nullptr, *su = c & 8 ? d : nullptr, *sc = c & 16 ? d : nullptr, *dJ = c & 32 ? d : nullptr;
      double *zl = c & 128 ? d : nullptr, *zh = c & 256 ? d : nullptr, *So = c & 512 ? d : nullptr;
      int32_t* fb = c & 64 ? i32 : nullptr;
      const size_t pi = (c >> 10) & 1, nsc = 3 * nc;
      const size_t mat = (pi ? B : 1) * n * n, cx = B * N * n, cu = B * (N - 1) * m, cz = B * (n + m), cs = B * N * n * n;
      StageLayout L;
      altro::stage_covariance(L, B, N, n, m, pi, nsc, S0, W, sx, su, sc, dJ, fb, zl, zh, So);
      expect(L.nslots == 10 && L.nslots <= StageLayout::MAX_SLOTS, "covariance: slots", c);
      size_t s = 0;
      slot_is(L, altro::COV_DJ, s, B * D, dJ, D, "covariance: dJ", c); s += B * D;
      slot_is(L, altro::COV_S0, s, S0 ? mat * D : 0, S0, D, "covariance: Sigma0", c); s += S0 ? mat * D : 0;
      slot_is(L, altro::COV_W, s, W ? mat * D : 0, W, D, "covariance: W", c); s += W ? mat * D : 0;
      slot_is(L, altro::COV_SX, s, sx ? cx * D : 0, sx, D, "covariance: sx", c); s += sx ? cx * D : 0;
      slot_is(L, altro::COV_SU, s, su ? cu * D : 0, su, D, "covariance: su", c); s += su ? cu * D : 0;
      slot_is(L, altro::COV_SC, s, sc ? B * nsc * D : 0, sc, D, "covariance: sc", c); s += sc ? B * nsc * D : 0;
      slot_is(L, altro::COV_ZLO, s, zl ? cz * D : 0, zl, D, "covariance: zmin_t", c); s += zl ? cz * D : 0;
      slot_is(L, altro::COV_ZHI, s, zh ? cz * D : 0, zh, D, "covariance: zmax_t", c); s += zh ? cz * D : 0;
      slot_is(L, altro::COV_SOUT, s, So ? cs * D : 0, So, D, "covariance: Sout", c); s += So ? cs * D : 0;
      slot_is(L, altro::COV_FB, s, B * I, fb, I, "covariance: fb", c); s += B * I;
      expect(L.bytes == s, "covariance: size", c);
      expect(L.slot[altro::COV_S0].in == S0 && L.slot[altro::COV_W].in == W && L.slot[altro::COV_FB].out == fb && L.slot[altro::COV_SOUT].out == So,
             "covariance: copies", c);
      arg_is(L, altro::COV_S0, "Sigma0", false, (pi ? B : 1) * n * n * D, "covariance: arg Sigma0", c);
      arg_is(L, altro::COV_W, "W", false, (pi ? B : 1) * n * n * D, "covariance: arg W", c);
      arg_is(L, altro::COV_SX, "sx", false, B * N * n * D, "covariance: arg sx", c);
      arg_is(L, altro::COV_SU, "su", false, B * (N - 1) * m * D, "covariance: arg su", c);
      arg_is(L, altro::COV_SC, "sc", false, B * nsc * D, "covariance: arg sc", c);
      arg_is(L, altro::COV_DJ, "dJ", false, B * D, "covariance: arg dJ", c);
      arg_is(L, altro::COV_FB, "fb", false, B * I, "covariance: arg fb", c);
      arg_is(L, altro::COV_ZLO, "zmin_t", false, B * (n + m) * D, "covariance: arg zmin_t", c);
      arg_is(L, altro::COV_ZHI, "zmax_t", false, B * (n + m) * D, "covariance: arg zmax_t", c);
      arg_is(L, altro::COV_SOUT, "Sout", false, B * N * n * n * D, "covariance: arg Sout", c);
    }
    // altro_batch_solution_vjp / _jvp: three inputs and three outputs only when given, fb has room either way; fb last (ints)
    for (int c = 0; c < 256; ++c) {
      const bool jvp = c & 128;   // the layout is one; the names are those of the form
      const double *ix = c & 1 ? d : nullptr, *iu = c & 2 ? d : nullptr, *i0 = c & 4 ? d : nullptr;
      double *o0 = c & 8 ? d : nullptr, *ox = c & 16 ? d : nullptr, *ou = c & 32 ? d : nullptr;
      int32_t* fb = c & 64 ? i32 : nullptr;
      const size_t R = B * nc, cx = R * N * n, cu = R * (N - 1) * m, c0 = R * n;
      StageLayout L;
      altro::stage_solution_sens(L, B, N, n, m, nc, jvp, ix, iu, i0, o0, ox, ou, fb);
      expect(L.nslots == 7 && L.nslots <= StageLayout::MAX_SLOTS, "solution sens: slots", c);
      size_t s = 0;
      slot_is(L, altro::SS_INX, s, ix ? cx * D : 0, ix, D, "solution sens: inx", c); s += ix ? cx * D : 0;
      slot_is(L, altro::SS_INU, s, iu ? cu * D : 0, iu, D, "solution sens: inu", c); s += iu ? cu * D : 0;
      slot_is(L, altro::SS_IN0, s, i0 ? c0 * D : 0, i0, D, "solution sens: in0", c); s += i0 ? c0 * D : 0;
      slot_is(L, altro::SS_O0, s, o0 ? c0 * D : 0, o0, D, "solution sens: o0", c); s += o0 ? c0 * D : 0;
      slot_is(L, altro::SS_OX, s, ox ? cx * D : 0, ox, D, "solution sens: ox", c); s += ox ? cx * D : 0;
      slot_is(L, altro::SS_OU, s, ou ? cu * D : 0, ou, D, "solution sens: ou", c); s += ou ? cu * D : 0;
      slot_is(L, altro::SS_FB, s, B * I, fb, I, "solution sens: fb", c); s += B * I;
      expect(L.bytes == s, "solution sens: size", c);
      expect(L.slot[altro::SS_INX].in == ix && L.slot[altro::SS_IN0].in == i0 && L.slot[altro::SS_OU].out == ou && L.slot[altro::SS_FB].out == fb,
             "solution sens: copies", c);
      arg_is(L, altro::SS_INX, jvp ? "vXref" : "gX", false, B * nc * N * n * D, "solution sens: arg gX / vXref", c);
      arg_is(L, altro::SS_INU, jvp ? "vUref" : "gU", false, B * nc * (N - 1) * m * D, "solution sens: arg gU / vUref", c);
      arg_is(L, altro::SS_IN0, "vx0", false, B * nc * n * D, "solution sens: arg vx0", c);
      arg_is(L, altro::SS_O0, "gx0", false, B * nc * n * D, "solution sens: arg gx0", c);
      arg_is(L, altro::SS_OX, jvp ? "dX" : "gXref", false, B * nc * N * n * D, "solution sens: arg gXref / dX", c);
      arg_is(L, altro::SS_OU, jvp ? "dU" : "gUref", false, B * nc * (N - 1) * m * D, "solution sens: arg gUref / dU", c);
      arg_is(L, altro::SS_FB, "fb", false, B * I, "solution sens: arg fb", c);
    }
    // altro_batch_solution_vjp_data: two seeds and eight outputs only when given, fb has room either way; fb last (ints);
    // gA, gB, gf hold N - 1 blocks per row with per_knot
    for (int c = 0; c < 4096; ++c) {
      const double *gX = c & 1 ? d : nullptr, *gU = c & 2 ? d : nullptr;
      double* out[8];
      for (int q = 0; q < 8; ++q) out[q] = c & (4 << q) ? d : nullptr;
      int32_t* fb = c & 1024 ? i32 : nullptr;
      const size_t pk = (c >> 11) & 1, R = B * nc, K1 = pk ? N - 1 : 1;
      const size_t cnt[8] = {R * n, R * n, R * m, R * (n + m), R * (n + m), R * K1 * n * n, R * K1 * n * m, R * K1 * n};
      const char* const name[8] = {"gQ", "gQf", "gR", "gzmin", "gzmax", "gA", "gB", "gf"};
      StageLayout L;
      altro::stage_solution_vjp_data(L, B, N, n, m, nc, pk, gX, gU, out, fb);
      expect(L.nslots == 11 && L.nslots <= StageLayout::MAX_SLOTS, "solution data: slots", c);
      size_t s = 0;
      slot_is(L, altro::SD_GX, s, gX ? R * N * n * D : 0, gX, D, "solution data: gX", c); s += gX ? R * N * n * D : 0;
      slot_is(L, altro::SD_GU, s, gU ? R * (N - 1) * m * D : 0, gU, D, "solution data: gU", c); s += gU ? R * (N - 1) * m * D : 0;
      for (int q = 0; q < 8; ++q) {
        slot_is(L, altro::SD_GQ + q, s, out[q] ? cnt[q] * D : 0, out[q], D, "solution data: output", c); s += out[q] ? cnt[q] * D : 0;
        arg_is(L, altro::SD_GQ + q, name[q], false, cnt[q] * D, "solution data: arg output", c);
        expect(L.slot[altro::SD_GQ + q].out == out[q] && L.slot[altro::SD_GQ + q].in == nullptr, "solution data: copies out", c);
      }
      slot_is(L, altro::SD_FB, s, B * I, fb, I, "solution data: fb", c); s += B * I;
      expect(L.bytes == s, "solution data: size", c);
      expect(altro::SD_GF == altro::SD_GQ + 7 && L.slot[altro::SD_GX].in == gX && L.slot[altro::SD_GU].in == gU && L.slot[altro::SD_FB].out == fb,
             "solution data: copies", c);
      arg_is(L, altro::SD_GX, "gX", false, B * nc * N * n * D, "solution data: arg gX", c);
      arg_is(L, altro::SD_GU, "gU", false, B * nc * (N - 1) * m * D, "solution data: arg gU", c);
      arg_is(L, altro::SD_FB, "fb", false, B * I, "solution data: arg fb", c);
    }
    // altro_batch_get_gain_active_set: mu_pass and codes only when given, fb has room either way; the bytes of codes last, so that
    // the doubles and the ints before them stay aligned
    for (int c = 0; c < 8; ++c) {
      static uint8_t u8[1];
      uint8_t* codes = c & 1 ? u8 : nullptr;
      double* mu = c & 2 ? d : nullptr;
      int32_t* fb = c & 4 ? i32 : nullptr;
      const size_t nc8 = B * N * (n + m);
      StageLayout L;
      altro::stage_gain_active_set(L, B, N, n, m, codes, mu, fb);
      expect(L.nslots == 3, "gain active set: slots", c);
      size_t s = 0;
      slot_is(L, altro::GA_MU, s, mu ? B * D : 0, mu, D, "gain active set: mu_pass", c); s += mu ? B * D : 0;
      slot_is(L, altro::GA_FB, s, B * I, fb, I, "gain active set: fb", c); s += B * I;
      slot_is(L, altro::GA_CODES, s, codes ? nc8 : 0, codes, 1, "gain active set: codes", c); s += codes ? nc8 : 0;
      expect(L.bytes == s, "gain active set: size", c);
      expect(L.slot[altro::GA_MU].out == mu && L.slot[altro::GA_FB].out == fb && L.slot[altro::GA_CODES].out == codes, "gain active set: copies", c);
      arg_is(L, altro::GA_MU, "mu_pass", false, B * D, "gain active set: arg mu_pass", c);
      arg_is(L, altro::GA_FB, "fb", false, B * I, "gain active set: arg fb", c);
      arg_is(L, altro::GA_CODES, "codes", false, B * N * (n + m), "gain active set: arg codes", c);
    }
    // altro_batch_cost_to_go: P0 [B][n][n], p0 [B][n], v0 [B], P [B][N][n][n], p [B][N][n], v [B][N], each only when given, in the
    // order of altro_ctg_out; fb has room either way and comes last (ints)
    for (int c = 0; c < 128; ++c) {
      double* P0 = c & 1 ? d : nullptr;
      double* p0 = c & 2 ? d : nullptr;
      double* v0 = c & 4 ? d : nullptr;
      double* P = c & 8 ? d : nullptr;
      double* p = c & 16 ? d : nullptr;
      double* v = c & 32 ? d : nullptr;
      int32_t* fb = c & 64 ? i32 : nullptr;
      double* const out[6] = {P0, p0, v0, P, p, v};
      StageLayout L;
      altro::stage_cost_to_go(L, B, N, n, out, fb);
      expect(L.nslots == 7, "cost to go: slots", c);
      size_t s = 0;
      slot_is(L, altro::CTG_P0, s, P0 ? B * n * n * D : 0, P0, D, "cost to go: P0", c); s += P0 ? B * n * n * D : 0;
      slot_is(L, altro::CTG_SP0, s, p0 ? B * n * D : 0, p0, D, "cost to go: p0", c); s += p0 ? B * n * D : 0;
      slot_is(L, altro::CTG_V0, s, v0 ? B * D : 0, v0, D, "cost to go: v0", c); s += v0 ? B * D : 0;
      slot_is(L, altro::CTG_P, s, P ? B * N * n * n * D : 0, P, D, "cost to go: P", c); s += P ? B * N * n * n * D : 0;
      slot_is(L, altro::CTG_SP, s, p ? B * N * n * D : 0, p, D, "cost to go: p", c); s += p ? B * N * n * D : 0;
      slot_is(L, altro::CTG_V, s, v ? B * N * D : 0, v, D, "cost to go: v", c); s += v ? B * N * D : 0;
      slot_is(L, altro::CTG_FB, s, B * I, fb, I, "cost to go: fb", c); s += B * I;
      expect(L.bytes == s, "cost to go: size", c);
      expect(L.slot[altro::CTG_P0].out == P0 && L.slot[altro::CTG_SP0].out == p0 && L.slot[altro::CTG_V0].out == v0 &&
                 L.slot[altro::CTG_P].out == P && L.slot[altro::CTG_SP].out == p && L.slot[altro::CTG_V].out == v &&
                 L.slot[altro::CTG_FB].out == fb,
             "cost to go: copies out", c);
      for (int q = 0; q < 7; ++q) expect(L.slot[q].in == nullptr, "cost to go: no input", c);
      arg_is(L, altro::CTG_P0, "P0", false, B * n * n * D, "cost to go: arg P0", c);
      arg_is(L, altro::CTG_SP0, "p0", false, B * n * D, "cost to go: arg p0", c);
      arg_is(L, altro::CTG_V0, "v0", false, B * D, "cost to go: arg v0", c);
      arg_is(L, altro::CTG_P, "P", false, B * N * n * n * D, "cost to go: arg P", c);
      arg_is(L, altro::CTG_SP, "p", false, B * N * n * D, "cost to go: arg p", c);
      arg_is(L, altro::CTG_V, "v", false, B * N * D, "cost to go: arg v", c);
      arg_is(L, altro::CTG_FB, "fb", false, B * I, "cost to go: arg fb", c);
    }
  }
  std::printf("stage_layout_check: %ld checks passed\n", checks);
  return 0;
}
