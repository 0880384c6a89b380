// stage_layout.h -- the argument table of each host/device twin pair (altro_batch_eval_policy, altro_batch_evaluate,
// altro_batch_evaluate_grad, altro_batch_evaluate_al, altro_batch_warm_start, altro_batch_simulate_policy,
// altro_batch_propagate_covariance, altro_batch_solution_vjp, altro_batch_solution_jvp, altro_batch_solution_vjp_data,
// altro_batch_get_gain_active_set, altro_batch_cost_to_go and their `_dev` forms): one function per
// pair names every array argument once, with its element count, type, direction and mode.  The `_dev` form validates the caller's
// pointers against the extents written here; the host twin puts the same arrays, in the same order, into the handle's staging buffer.
// Plain host arithmetic, no HIP: altro_batch.hip's TwinArgs adds the validation and the copies, and tools/stage_layout_check.cpp runs
// this file alone on the CPU against names, extents, sizes and offsets written out by hand.
#pragma once
#include <cassert>
#include <cstddef>
#include <cstdint>

namespace altro {

// The array arguments of one call; in the staging buffer they are consecutive sub-arrays in the order they are added.
struct StageLayout {
  enum Mode {
    OPTIONAL,   // room only when the caller passes the array; the kernels get null otherwise
    RESERVED,   // room either way; the kernels get null when the caller passes no array
    KEPT        // room either way, and the kernels get the sub-array either way (they read it themselves)
  };
  struct Slot {
    const char* name;    // as include/altro_batch.h names the argument (a string literal)
    bool required;       // the `_dev` form refuses null
    size_t extent;       // count * sizeof(T): what the `_dev` form validates, kept when there is no room
    size_t off, bytes;   // bytes = 0: no room
    const void* in;      // copied to the device before the launch, or null
    void* out;           // copied back after it, or null
    bool dev;            // the kernels get the sub-array
    const void* arg() const { return in ? in : out; }   // the caller's own pointer
  };
  static constexpr int MAX_SLOTS = 14;
  Slot slot[MAX_SLOTS] = {};
  int nslots = 0;
  size_t bytes = 0;

  template <class T>
  void add(const char* name, size_t count, const T* in, T* out, Mode mode, bool required = false) {
    const bool present = in != nullptr || out != nullptr;
    assert(nslots < MAX_SLOTS);   // (a twin with more sub-arrays raises MAX_SLOTS)
    Slot& s = slot[nslots++];
    s.name = name;
    s.required = required;
    s.extent = count * sizeof(T);
    s.off = bytes;
    s.bytes = (present || mode != OPTIONAL) ? s.extent : 0;
    s.in = in;
    s.out = out;
    s.dev = present || mode == KEPT;
    bytes += s.bytes;
  }
};

// the slots of each pair, in the order of its layout
enum { EP_X, EP_U, EP_KNOT, EP_FB };
inline void stage_eval_policy(StageLayout& L, size_t B, size_t n, size_t m, const double* x, const int32_t* knot, double* u, int32_t* fb) {
  L.add<double>("x", B * n, x, nullptr, StageLayout::OPTIONAL, true);
  L.add<double>("u", B * m, nullptr, u, StageLayout::OPTIONAL, true);
  L.add<int32_t>("knot", B, knot, nullptr, StageLayout::RESERVED);
  L.add<int32_t>("fb", B, nullptr, fb, StageLayout::RESERVED);
}

enum { EV_J, EV_CMAX, EV_DEFECT, EV_U, EV_X, EV_X0, EV_XOUT };
inline void stage_evaluate(StageLayout& L, size_t B, size_t N, size_t n, size_t m, size_t ncand, const double* U, const double* X,
                           const double* x0, double* J, double* c_max, double* defect, double* Xout) {
  const size_t R = B * ncand, cu = R * (N - 1) * m, cx = R * N * n;
  L.add<double>("J", R, nullptr, J, StageLayout::RESERVED);
  L.add<double>("c_max", R, nullptr, c_max, StageLayout::RESERVED);
  L.add<double>("defect", R, nullptr, defect, StageLayout::RESERVED);
  L.add<double>("U", cu, U, nullptr, StageLayout::OPTIONAL);
  L.add<double>("X", cx, X, nullptr, StageLayout::OPTIONAL);
  L.add<double>("x0", B * n, x0, nullptr, StageLayout::OPTIONAL);
  L.add<double>("Xout", cx, nullptr, Xout, StageLayout::OPTIONAL);
}

enum { EG_J, EG_P, EG_GU, EG_GX0, EG_U, EG_X0, EG_XOUT };
inline void stage_evaluate_grad(StageLayout& L, size_t B, size_t N, size_t n, size_t m, size_t ncand, const double* U, const double* x0,
                                double* J, double* P, double* gU, double* gx0, double* Xout) {
  const size_t R = B * ncand, cu = R * (N - 1) * m;
  L.add<double>("J", R, nullptr, J, StageLayout::RESERVED);
  L.add<double>("P", R, nullptr, P, StageLayout::RESERVED);
  L.add<double>("gU", cu, nullptr, gU, StageLayout::OPTIONAL);
  L.add<double>("gx0", R * n, nullptr, gx0, StageLayout::OPTIONAL);
  L.add<double>("U", cu, U, nullptr, StageLayout::OPTIONAL, true);
  L.add<double>("x0", B * n, x0, nullptr, StageLayout::OPTIONAL);
  L.add<double>("Xout", R * N * n, nullptr, Xout, StageLayout::OPTIONAL);
}

// out[AL_LA .. AL_XOUT]: the twelve pointers of altro_al_out in the order of the struct; every sub-array only when given
enum { AL_LA, AL_J, AL_GU, AL_GX0, AL_GXREF, AL_GUREF, AL_GQ, AL_GQF, AL_GR, AL_GZMIN, AL_GZMAX, AL_XOUT, AL_U, AL_X0, AL_SLOTS };
inline void stage_evaluate_al(StageLayout& L, size_t B, size_t N, size_t n, size_t m, size_t ncand, const double* U, const double* x0,
                              double* const (&out)[12]) {
  const size_t R = B * ncand, cu = R * (N - 1) * m, cx = R * N * n;
  const char* const name[12] = {"LA", "J", "gU", "gx0", "gXref", "gUref", "gQ", "gQf", "gR", "gzmin", "gzmax", "Xout"};
  const size_t count[12] = {R, R, cu, R * n, cx, cu, R * n, R * n, R * m, R * (n + m), R * (n + m), cx};
  for (int i = 0; i < 12; ++i) L.add<double>(name[i], count[i], nullptr, out[i], StageLayout::OPTIONAL);
  L.add<double>("U", cu, U, nullptr, StageLayout::OPTIONAL);
  L.add<double>("x0", B * n, x0, nullptr, StageLayout::OPTIONAL);
}

enum { WS_J, WS_CMAX, WS_U, WS_CHOSEN };
inline void stage_warm_start(StageLayout& L, size_t B, size_t N, size_t m, size_t ncand, size_t inc, const double* U, int32_t* chosen,
                             double* J, double* c_max) {
  const size_t R1 = B * (ncand + inc);
  L.add<double>("J", R1, nullptr, J, StageLayout::KEPT);   // (the install kernel reads the merits)
  L.add<double>("c_max", R1, nullptr, c_max, StageLayout::KEPT);
  L.add<double>("U", B * ncand * (N - 1) * m, U, nullptr, StageLayout::KEPT, true);
  L.add<int32_t>("chosen", B, nullptr, chosen, StageLayout::KEPT);
}

enum { SIM_J, SIM_CMAX, SIM_DXMAX, SIM_X0, SIM_W, SIM_XOUT, SIM_UOUT, SIM_FB };
inline void stage_simulate(StageLayout& L, size_t B, size_t N, size_t n, size_t m, size_t nsamp, const double* x0, const double* w, double* J,
                           double* c_max, double* dx_max, int32_t* fb, double* Xout, double* Uout) {
  const size_t R = B * nsamp;
  L.add<double>("J", R, nullptr, J, StageLayout::RESERVED);
  L.add<double>("c_max", R, nullptr, c_max, StageLayout::RESERVED);
  L.add<double>("dx_max", R, nullptr, dx_max, StageLayout::RESERVED);
  L.add<double>("x0", R * n, x0, nullptr, StageLayout::OPTIONAL);
  L.add<double>("w", R * (N - 1) * n, w, nullptr, StageLayout::OPTIONAL);
  L.add<double>("Xout", R * N * n, nullptr, Xout, StageLayout::OPTIONAL);
  L.add<double>("Uout", R * (N - 1) * m, nullptr, Uout, StageLayout::OPTIONAL);
  L.add<int32_t>("fb", B, nullptr, fb, StageLayout::RESERVED);
}

enum { COV_DJ, COV_S0, COV_W, COV_SX, COV_SU, COV_SC, COV_ZLO, COV_ZHI, COV_SOUT, COV_FB };
inline void stage_covariance(StageLayout& L, size_t B, size_t N, size_t n, size_t m, size_t per_instance, size_t nsc, const double* Sigma0,
                             const double* W, double* sx, double* su, double* sc, double* dJ, int32_t* fb, double* zmin_t, double* zmax_t,
                             double* Sout) {
  const size_t mat = (per_instance ? B : 1) * n * n;
  L.add<double>("dJ", B, nullptr, dJ, StageLayout::RESERVED);
  L.add<double>("Sigma0", mat, Sigma0, nullptr, StageLayout::OPTIONAL);
  L.add<double>("W", mat, W, nullptr, StageLayout::OPTIONAL);
  L.add<double>("sx", B * N * n, nullptr, sx, StageLayout::OPTIONAL);
  L.add<double>("su", B * (N - 1) * m, nullptr, su, StageLayout::OPTIONAL);
  L.add<double>("sc", B * nsc, nullptr, sc, StageLayout::OPTIONAL);
  L.add<double>("zmin_t", B * (n + m), nullptr, zmin_t, StageLayout::OPTIONAL);
  L.add<double>("zmax_t", B * (n + m), nullptr, zmax_t, StageLayout::OPTIONAL);
  L.add<double>("Sout", B * N * n * n, nullptr, Sout, StageLayout::OPTIONAL);
  L.add<int32_t>("fb", B, nullptr, fb, StageLayout::RESERVED);
}

// altro_batch_solution_vjp / _jvp (one layout: the JVP has no s_0, the VJP no xi_0), named as the form at hand names them
enum { SS_INX, SS_INU, SS_IN0, SS_O0, SS_OX, SS_OU, SS_FB };
inline void stage_solution_sens(StageLayout& L, size_t B, size_t N, size_t n, size_t m, size_t nseed, bool jvp, const double* inx,
                                const double* inu, const double* in0, double* o0, double* ox, double* ou, int32_t* fb) {
  const size_t R = B * nseed;
  L.add<double>(jvp ? "vXref" : "gX", R * N * n, inx, nullptr, StageLayout::OPTIONAL);
  L.add<double>(jvp ? "vUref" : "gU", R * (N - 1) * m, inu, nullptr, StageLayout::OPTIONAL);
  L.add<double>("vx0", R * n, in0, nullptr, StageLayout::OPTIONAL);
  L.add<double>("gx0", R * n, nullptr, o0, StageLayout::OPTIONAL);
  L.add<double>(jvp ? "dX" : "gXref", R * N * n, nullptr, ox, StageLayout::OPTIONAL);
  L.add<double>(jvp ? "dU" : "gUref", R * (N - 1) * m, nullptr, ou, StageLayout::OPTIONAL);
  L.add<int32_t>("fb", B, nullptr, fb, StageLayout::RESERVED);
}

// out[0 .. 7]: the eight pointers of altro_sens_data_out in the order of the struct; every sub-array only when given.  K1 = N - 1
// blocks of gA, gB, gf per row with per_knot, else one.
enum { SD_GX, SD_GU, SD_GQ, SD_GQF, SD_GR, SD_GZMIN, SD_GZMAX, SD_GA, SD_GB, SD_GF, SD_FB };
inline void stage_solution_vjp_data(StageLayout& L, size_t B, size_t N, size_t n, size_t m, size_t nseed, size_t per_knot, const double* gX,
                                    const double* gU, double* const (&out)[8], int32_t* fb) {
  const size_t R = B * nseed, K1 = per_knot ? N - 1 : 1;
  const char* const name[8] = {"gQ", "gQf", "gR", "gzmin", "gzmax", "gA", "gB", "gf"};
  const size_t count[8] = {R * n, R * n, R * m, R * (n + m), R * (n + m), R * K1 * n * n, R * K1 * n * m, R * K1 * n};
  L.add<double>("gX", R * N * n, gX, nullptr, StageLayout::OPTIONAL);
  L.add<double>("gU", R * (N - 1) * m, gU, nullptr, StageLayout::OPTIONAL);
  for (int i = 0; i < 8; ++i) L.add<double>(name[i], count[i], nullptr, out[i], StageLayout::OPTIONAL);
  L.add<int32_t>("fb", B, nullptr, fb, StageLayout::RESERVED);
}

// codes last: the doubles and the ints stay aligned whatever its byte count
enum { GA_MU, GA_FB, GA_CODES };
inline void stage_gain_active_set(StageLayout& L, size_t B, size_t N, size_t n, size_t m, uint8_t* codes, double* mu_pass, int32_t* fb) {
  const size_t nc = B * N * (n + m);
  L.add<double>("mu_pass", B, nullptr, mu_pass, StageLayout::OPTIONAL);
  L.add<int32_t>("fb", B, nullptr, fb, StageLayout::RESERVED);
  L.add<uint8_t>("codes", nc, nullptr, codes, StageLayout::OPTIONAL);
}

// out[0 .. 5]: the six pointers of altro_ctg_out in the order of the struct; every sub-array only when given
enum { CTG_P0, CTG_SP0, CTG_V0, CTG_P, CTG_SP, CTG_V, CTG_FB };
inline void stage_cost_to_go(StageLayout& L, size_t B, size_t N, size_t n, double* const (&out)[6], int32_t* fb) {
  const char* const name[6] = {"P0", "p0", "v0", "P", "p", "v"};
  const size_t count[6] = {B * n * n, B * n, B, B * N * n * n, B * N * n, B * N};
  for (int i = 0; i < 6; ++i) L.add<double>(name[i], count[i], nullptr, out[i], StageLayout::OPTIONAL);
  L.add<int32_t>("fb", B, nullptr, fb, StageLayout::RESERVED);
}

}  // namespace altro
