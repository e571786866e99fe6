// TEST-ONLY: the per-environment body of k_reset_envs (mjb_device.hpp reset_env_state) compiled for the host with g++ -DMJB_HOST_EMU,
// driven over a batch the way the kernel drives it (mask, global index env0 + e, episode number + 1).  Used by
// tests/test_reset_envs_host.py; not part of the product library.
#define MJB_HOST_EMU 1
#include "../mujoco_template_amd/csrc/mjb_device.hpp"

using namespace mjb;

template <typename TS>
static void run(int batch, int nq, int nv, int nu, int njnt, const int* jt, const int* jq, const int* jd, const double* qpos, const double* qvel,
                const double* ctrl, unsigned seed, double qn, double qv, unsigned env0, const unsigned char* mask, unsigned* episode,
                TS* o_qpos, TS* o_qvel, TS* o_ctrl, TS* o_qacc, TS* o_qws) {
  ResetSpec r;
  r.nq = nq; r.nv = nv; r.nu = nu; r.njnt = njnt; r.jnt_type = jt; r.jnt_qposadr = jq; r.jnt_dofadr = jd;
  r.qpos = qpos; r.qvel = qvel; r.ctrl = ctrl; r.time = 0; r.seed = seed; r.qpos_noise = qn; r.qvel_noise = qv;
  for (int e = 0; e < batch; e++) {
    if (mask && !mask[e]) continue;
    reset_env_state<TS>(r, env0 + (unsigned)e, episode[e], o_qpos + (size_t)e * nq, o_qvel + (size_t)e * nv, o_ctrl + (size_t)e * nu,
                        o_qacc + (size_t)e * nv, o_qws + (size_t)e * nv);
    episode[e]++;
  }
}

extern "C" {
int reset_envs_f64(int batch, int nq, int nv, int nu, int njnt, const int* jt, const int* jq, const int* jd, const double* qpos, const double* qvel,
                   const double* ctrl, unsigned seed, double qn, double qv, unsigned env0, const unsigned char* mask, unsigned* episode,
                   double* o_qpos, double* o_qvel, double* o_ctrl, double* o_qacc, double* o_qws) {
  run<double>(batch, nq, nv, nu, njnt, jt, jq, jd, qpos, qvel, ctrl, seed, qn, qv, env0, mask, episode, o_qpos, o_qvel, o_ctrl, o_qacc, o_qws);
  return 0;
}
int reset_envs_f32(int batch, int nq, int nv, int nu, int njnt, const int* jt, const int* jq, const int* jd, const double* qpos, const double* qvel,
                   const double* ctrl, unsigned seed, double qn, double qv, unsigned env0, const unsigned char* mask, unsigned* episode,
                   float* o_qpos, float* o_qvel, float* o_ctrl, float* o_qacc, float* o_qws) {
  run<float>(batch, nq, nv, nu, njnt, jt, jq, jd, qpos, qvel, ctrl, seed, qn, qv, env0, mask, episode, o_qpos, o_qvel, o_ctrl, o_qacc, o_qws);
  return 0;
}
}
