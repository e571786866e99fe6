/*
 * mjbatch.h — C ABI of the MI355X-native batched MuJoCo step/rollout engine.
 *
 * This is the drop-in boundary for the reference's per-step physics path.  The
 * reference (pure Python) reaches its physics through the pybind11 surface of the
 * third-party `mujoco` package (stub: reference mujoco_template/mujoco.pyi:1-75);
 * each entry point below names the reference call site it replaces.  Handles are
 * opaque, arguments are plain pointers and sizes, every function returns 0 on
 * success or a negative status and leaves a message for mjb_last_error().
 * All functions on one mjbData are NOT re-entrant (reference semantics are
 * single-threaded); launches go to the stream set with mjb_set_stream().
 *
 * There is no CPU fallback: without a HIP device mjb_data_create() fails.
 */
#ifndef MJBATCH_H
#define MJBATCH_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mjbModel mjbModel;
typedef struct mjbData mjbData;
typedef struct mjbObsSpec mjbObsSpec;

#define MJB_OK 0
#define MJB_ERR_ARG (-1)     /* bad argument / unknown name        -> ConfigError      */
#define MJB_ERR_MODEL (-2)   /* model table rejected                -> ValueError       */
#define MJB_ERR_DEVICE (-3)  /* HIP error / no device               -> TemplateError    */
#define MJB_ERR_LOOKUP (-4)  /* index out of range                  -> NameLookupError  */

#define MJB_F32 0
#define MJB_F64 1

/* ctrl source of a fused rollout */
#define MJB_CTRL_KEEP 0    /* use data.ctrl as is (host controller wrote it)  */
#define MJB_CTRL_ZERO 1    /* ZeroController, reference controllers.py:12-25 */
#define MJB_CTRL_RANDOM 2  /* uniform random ctrl, Philox(seed; env, step, actuator) */
#define MJB_CTRL_FEEDBACK 3 /* ctrl = clip(u0 - K [q (-) q0; qvel - v0]): the LQR law of the reference's examples
                               (examples/humanoid/controllers/lqr.py:147-170), gains set by mjb_set_feedback */

const char* mjb_last_error(void);
int mjb_device_count(void);

/* ---- model: replaces MjModel.from_xml_* (reference model.py:22-37).  mjb_model_load_xml* compile MJCF inside the library;
 * mjb_model_create takes an already compiled model as a table of named arrays (dtype 0 = float64, 1 = int32, 2 = bytes) whose
 * names follow mjModel (what mjb_model_load_xml* and mjb_model_load build internally). ---- */
int mjb_model_create(int nfield, const char* const* names, const void* const* ptrs, const int* dtypes,
                     const long* counts, mjbModel** out);
/* MjModel.from_xml_path / from_xml_string (reference model.py:22-27) in the library itself: the MJCF-subset compiler
 * (csrc/mjb_mjcf.cpp, host C++) -> the same table -> mjb_model_create.  Anything outside the supported subset is rejected with
 * MJB_ERR_MODEL and a message naming it (the host front raises ValueError, as mujoco's compiler does).  base_dir resolves
 * <include file=...>. */
int mjb_model_load_xml(const char* path, mjbModel** out);
int mjb_model_load_xml_string(const char* xml_text, const char* base_dir, mjbModel** out);
void mjb_model_free(mjbModel* m);
/* model.opt.disableactuator bit mask, reference model.py:88-93 */
int mjb_model_set_disableactuator(mjbModel* m, int mask);
/* solver knobs (mjOption.iterations / tolerance) */
int mjb_model_set_solver(mjbModel* m, int iterations, double tolerance);

/* object names: mj_name2id / mj_id2name (reference observations.py:80-84, jacobians.py:39-75, logging.py:88-126, model.py:64).
 * objtype = MuJoCo's mjtObj code (1 body, 2 xbody, 3 joint, 5 geom, 6 site, 18 tendon, 19 actuator, 20 sensor, 24 key);
 * name2id returns -1 when the name is unknown (the host front raises NameLookupError), id2name NULL for unnamed / out of range.
 * The names cross mjb_model_create as table fields "names_<objtype>" of dtype 2 (bytes: NUL-terminated names in id order). */
int mjb_model_name2id(const mjbModel* m, int objtype, const char* name);
const char* mjb_model_id2name(const mjbModel* m, int objtype, int id);
/* any field of the compiled model by its mjModel name ("nq", "nv", "actuator_ctrlrange", "jnt_type", ...): host pointer valid for the
 * model's lifetime, element count and dtype (0 float64, 1 int32, 2 bytes) — the model.nq / model.actuator_* / model.jnt_* attribute
 * reads of the reference (mujoco.pyi:7-49, compat.py:64-121) for a host that is not Python */
int mjb_model_field(const mjbModel* m, const char* name, const void** ptr, long* count, int* dtype);
/* enumeration of the same fields: 0 and the field's name / pointer / count / dtype for 0 <= index < n, otherwise n (the field count) */
int mjb_model_field_at(const mjbModel* m, int index, const char** name, const void** ptr, long* count, int* dtype);
/* MjModel.from_binary_path / mj_saveModel (reference model.py:28-31, :49): the compiled table in a flat binary file ("MJBM0001").
 * A host without the Python MJCF compiler loads a model compiled once elsewhere. */
int mjb_model_save(const mjbModel* m, const char* path);
int mjb_model_load(const char* path, mjbModel** out);

/* mj_integratePos(m, qpos, qvel, dt) / mj_differentiatePos(m, qvel, dt, qpos1, qpos2) (reference linearization.py:12,67,77,
 * examples/humanoid/controllers/lqr.py:153, examples/drone2/main.py:404-406): in place on CALLER-OWNED HOST vectors, float64,
 * batched: qpos [batch, nq], qvel [batch, nv] row-major.  qvel_out = (qpos2 (-) qpos1) / dt in the tangent space. */
int mjb_integrate_pos(const mjbModel* m, int batch, double* qpos, const double* qvel, double dt);
int mjb_differentiate_pos(const mjbModel* m, int batch, double* qvel_out, double dt, const double* qpos1, const double* qpos2);

/* ---- data: replaces MjData(model) (reference model.py:16-19) for `batch` independent replicas.
 * dtype: MJB_F32 (product path) or MJB_F64.  lanes: lanes per environment (8, 16, 64; 0 = auto).
 * nconmax / nefcmax: per-environment contact / constraint-row caps held in LDS (0 = default).
 * env0: global index of this shard's first environment (keeps random ctrl shard-invariant). ---- */
int mjb_data_create(mjbModel* m, int batch, int dtype, int lanes, int nconmax, int nefcmax, int device, int env0, mjbData** out);
void mjb_data_free(mjbData* d);
int mjb_set_stream(mjbData* d, void* hip_stream);
int mjb_sync(mjbData* d);
/* Engine failures cross the ABI (reference convention: mujoco raises FatalError / mujoco_template raises TemplateError,
 * exceptions.py:4-21 - nothing is ever silently wrong).  Sticky flag word of the batch, bit 0 contacts dropped, 1 constraint rows
 * dropped (per-environment LDS caps exceeded: truncated physics, COUNTED per environment by mjb_get_counters), 2 bad-state auto-reset
 * (mj_checkPos/Vel/Acc), 3 a ticket-mode launch timed out waiting for a state hand-over.  mjb_engine_flags waits for the stream and
 * reports the word (the kernels keep it in pinned host memory: no copy).  Bit 3 is an ERROR: from the first synchronising call
 * after it was raised (mjb_sync, mjb_get_array, mjb_get_counters, mjb_sync_to_host, mjb_step_host*) and at the entry of every
 * further launch (mjb_step, mjb_rollout, mjb_forward ...) the library returns MJB_ERR_DEVICE until mjb_reset clears the flags; the
 * environments concerned were NOT advanced (their arrays hold the state the failed launch started from). */
int mjb_engine_flags(mjbData* d, int* flags_out);
/* the same word WITHOUT waiting for the stream (device-resident loops: no host synchronisation): what the launches that have finished
 * so far raised, read from the pinned words the kernels store (reference FatalError / warning surfacing, env.py:186-190) */
int mjb_engine_flags_peek(mjbData* d, int* flags_out);
int mjb_data_info(mjbData* d, int* batch, int* dtype, int* lanes, int* nconmax, int* nefcmax, int* lds_bytes_per_env);

/* device pointer of a [batch, n] state array: qpos qvel ctrl qacc qacc_warmstart (dtype of the data),
 * time (float64 [batch]), xpos xquat xipos site_xpos geom_xpos subtree_com sensordata qfrc_inverse actuator_moment, counters (int32 [batch, 8]),
 * episode (resets per environment by mjb_reset_envs: uint32 bits, reported as int32 [batch, 1]) */
int mjb_array_ptr(mjbData* d, const char* name, void** dev_ptr, long* per_env, int* dtype);
/* host <-> device copies with conversion to/from float64 (state snapshot/restore, reference state_utils.py:9-31); "episode" is
 * read-only and mjb_get_array widens its uint32 values (counters: mjb_get_counters) */
int mjb_get_array(mjbData* d, const char* name, double* host_out);
int mjb_set_array(mjbData* d, const char* name, const double* host_in);
int mjb_get_counters(mjbData* d, int* host_out /* [batch, 8] */);

/* ---- host mirror ("host_view"): the zero-copy numpy views data.qpos / qvel / ctrl / qacc / qacc_warmstart / time of the reference
 * (mujoco.pyi:51-75; observations with copy=False alias them, tests/test_mujoco_template.py:241-252) as ONE pinned float64 block
 * per data object.  mjb_host_view returns the address of one field's [batch, n] slice (valid for the data's lifetime);
 * mjb_sync_to_host refreshes the whole block with one pack kernel + ONE device-to-host copy + one stream sync;
 * mjb_sync_to_device uploads the fields named in field_mask (bit 0 qpos, 1 qvel, 2 ctrl, 3 qacc, 4 qacc_warmstart, 5 time) after the
 * host edited them in place (data.ctrl[:] = ..., what every reference controller does);
 * mjb_step_host = sync_to_device(field_mask) + nstep x mj_step (nstep = 0: mj_forward) + sync_to_host in one call: the body of the
 * reference's host-driven loop (env.py:186-190, runtime.py:631-663) costs one library call per step. ---- */
/* name "engine_flags": ONE double behind the state, refreshed by the same copy: sticky bits 0 contacts dropped, 1 constraint rows dropped
 * (per-environment LDS caps exceeded), 2 bad-state auto-reset, 3 hand-over timed out (see mjb_engine_flags) — the whole-batch OR of what
 * mjb_get_counters details per environment */
int mjb_host_view(mjbData* d, const char* name, double** host_ptr, long* per_env);
int mjb_sync_to_host(mjbData* d);
int mjb_sync_to_device(mjbData* d, int field_mask);
int mjb_step_host(mjbData* d, int nstep, int field_mask);
/* Edit detection inside the library: the reference's controllers write data.ctrl / qpos / qvel IN PLACE through the numpy views
 * (control.py:26-32, examples/drone2/main.py:393-397), so "what did the host change since the block was last refreshed" is a comparison
 * of the pinned block with a library-owned shadow copy.  mjb_mirror_edited_mask: bit k set = field k differs from the shadow;
 * mjb_mirror_commit: the shadow takes the block's current content for the fields in field_mask (after a refresh or an upload);
 * mjb_step_host_auto = [compare != 0: edited mask, else 0] + mjb_step_host(nstep, mask) + commit(all): ONE call per reference-style
 * Env.step; *mask_out (may be NULL) receives the mask that was uploaded. */
int mjb_mirror_edited_mask(mjbData* d, int* mask_out);
int mjb_mirror_commit(mjbData* d, int field_mask);
int mjb_step_host_auto(mjbData* d, int nstep, int compare, int* mask_out);

/* ---- per-model specialised kernels (no reference counterpart: the reference's MjModel is interpreted by one pre-built C library;
 * here the structural sizes of the compiled model and the LDS layout offsets can be folded into a kernel, and the model itself baked
 * in as constants).  Three kinds, each with results bitwise those of the generic kernel it replaces:
 *   MJB_KERNEL_STEP   the fp32 step kernel (float32 data objects only);
 *   MJB_KERNEL_FD     the float64 finite-difference kernel behind mjb_transition_fd (k_fd<double, TS, G>: float64 layout);
 *   MJB_KERNEL_STEP2  the TWO-WAVE step kernel that stepping launches use on small batches (one environment per 128-thread workgroup,
 *                     the independent phases of a step side by side on its two wavefronts; fp32, one wave per environment,
 *                     nv <= 32, Euler).  mjb_step_schedule()[5] tells whether a launch used it; MJB_TWO_WAVE=0 / 1 forces it off / on.
 * mjb_kernel_source writes a data object's translation unit of that kind, mjb_model_kernel_source the one a data object created
 * with these arguments would get (no device needed: a build step); both return its length (call with buf = NULL to size it) or -1
 * where the kind does not apply or mjb_data_create would reject the arguments.  Compile it for gfx950 with
 * `hipcc --genco -I <csrc>` (mujoco_template_amd/_capi.py does, cached in-tree) and hand the code object to mjb_kernel_load: every
 * later launch of that kernel on this data object uses it.  The generic kernels stay the default and the fallback. ---- */
#define MJB_KERNEL_STEP 1
#define MJB_KERNEL_FD 2
#define MJB_KERNEL_STEP2 3
long mjb_model_kernel_source(mjbModel* m, int kind, int dtype, int lanes, int nconmax, int nefcmax, char* buf, long cap);
long mjb_kernel_source(mjbData* d, int kind, char* buf, long cap);
int mjb_kernel_load(mjbData* d, int kind, const void* code_object, long nbytes);
int mjb_kernel_unload(mjbData* d, int kind);

/* mj_resetData / mj_resetDataKeyframe (reference model.py:59-71); key < 0 = qpos0 */
int mjb_reset(mjbData* d, int key);
/* mj_forward (reference model.py:53-54): fills qacc and the kinematic outputs */
int mjb_forward(mjbData* d);
/* Per-environment mj_resetData / mj_resetDataKeyframe (reference model.py:59-71) and mj_forward (reference model.py:53-54), both on the
 * data's stream, the mask read on the device (no host synchronisation).  mask_dev: [batch] bytes in device-accessible memory, non-zero =
 * this environment; NULL = every environment.  mjb_reset_envs: key < 0 = qpos0; qacc = qacc_warmstart = 0, counters zeroed, time of the
 * keyframe, array "episode" (uint32 [batch], zeroed at creation) + 1; optional uniform noise (float64, rounded once to the data dtype):
 * dq = qpos_noise (2u - 1) applied as mj_integratePos(qpos, dq, 1) over the nv dofs, qvel += qvel_noise (2u - 1), u a Philox4x32-10
 * draw keyed (seed, 0x5EED) with counter (env0 + e, episode[e] before the increment, i, 1 for qpos / 2 for qvel).  Unlike mjb_reset the
 * sticky engine flags are left alone.  mjb_forward_envs: environments outside the mask keep every array. */
int mjb_reset_envs(mjbData* d, int key, const unsigned char* mask_dev, unsigned seed, double qpos_noise, double qvel_noise);
int mjb_forward_envs(mjbData* d, const unsigned char* mask_dev);
/* mj_inverse (reference setpoints.py:29-31 steady_ctrl0, examples/humanoid/controllers/lqr.py:57-70): inverse dynamics at the
 * current (qpos, qvel, qacc) of every environment -> array "qfrc_inverse" [batch, nv]; the same pass fills
 * "actuator_moment" [batch, nu, nv] (dense form of data.actuator_moment, which setpoints.py:40-47 densifies).  State is not advanced. */
int mjb_inverse(mjbData* d);
/* nstep x mj_step (reference model.py:56-57, env.py:190), ctrl taken from data.ctrl */
int mjb_step(mjbData* d, int nstep);
/* fused rollout = the body of runtime.iterate_passive (reference runtime.py:631-663) for a device-side
 * controller: nstep x [ctrl <- mode, mj_step]; when spec != NULL the flat observation of every
 * `obs_every`-th step is written to obs_out_dev[(nstep/obs_every), batch, dim] (dtype of the data). */
int mjb_rollout(mjbData* d, int nstep, int ctrl_mode, unsigned seed, unsigned step0, double ctrl_scale,
                const mjbObsSpec* spec, void* obs_out_dev, int obs_every);

/* open-loop rollout: nstep x [ctrl <- ctrl_dev[s*step_stride + e*env_stride + a], mj_step]; ctrl_dev device memory in the data's
 * dtype; strides in elements, >= 0 (0 = broadcast); spec / obs_out_dev / obs_every as in mjb_rollout.
 * Replaces the controller-in-the-loop body of the reference (runtime.py:631-663 calling control.py:26-32) when the controls are known
 * in advance (sampling planners, shooting): one launch for the whole rollout, s = 0 .. nstep-1 the step of this call, e the data's own
 * (shard-local) environment index.  With an obs spec of qpos | qvel | sensordata | time and obs_every = 1, ring row t is the state
 * after step t with the sensors of that step's forward pass (the order of mujoco.rollout).  data.ctrl ends as the last applied row.
 * Checked before anything is launched (MJB_ERR_ARG, state and engine flags untouched): nstep >= 1, strides >= 0, ctrl_dev non-NULL
 * when nu > 0, device-accessible memory of the data's device (hipPointerGetAttributes), and the highest element read,
 * (nstep-1)*step_stride + (batch-1)*env_stride + nu-1, inside the allocation behind ctrl_dev (hipMemGetAddressRange). */
int mjb_rollout_ctrl(mjbData* d, int nstep, const void* ctrl_dev, long step_stride, long env_stride,
                     const mjbObsSpec* spec, void* obs_out_dev, int obs_every);

/* ---- per-environment model parameters (domain randomisation): these fields may differ between the environments of one data object.
 * Each is stored as [batch, n] float64 on the data's device (plus an fp32 copy, (float)double, for float32 data); every kernel that
 * runs environment e's physics (step in both work maps, two-wave step, forward / forward_envs / inverse, host-driven steps, rollouts,
 * finite differences, Jacobians) reads e's row of a batched field and the model table of the others.
 *   name               n per environment   bit of the mask
 *   body_mass          nbody               0 (MJB_PRM_BODY_MASS)
 *   body_inertia       nbody * 3           1
 *   dof_damping        nv                  2
 *   dof_armature       nv                  3
 *   actuator_gear      nu * 6              4
 *   actuator_gainprm   nu * 3              5
 *   actuator_biasprm   nu * 3              6
 *   geom_friction      ngeom * 3           7
 *   gravity            3                   8
 * Semantics: those of MuJoCo when a field of mjModel is edited without mj_setConst.  Per environment the library re-derives only what
 * the compiler derives from these fields, the same way: body_subtreemass = sum of body_mass over the subtree, and the friction of a
 * collision pair = element-wise max of its two geoms' friction, stored [f0, f0, f1, f2, f2].  body_invweight0, dof_invweight0,
 * meaninertia, the pair's translational invweight term and every constraint K / B constant stay those of the compiled model.
 * Batching dof_damping on a model whose compiled damping is all zero switches that data's Euler step to the implicit-damping path.
 * Parameters are model, not state: mjb_reset, mjb_reset_envs and the ticket-map hand-over leave them alone.  A specialised kernel is
 * built for one set of batched fields (its source defines MJB_SPEC_PARAMS when the set is not empty): a call that changes the set
 * unloads the specialised kernels built for another set (the generic kernels run until the caller loads new ones), and
 * mjb_kernel_load rejects a code object built for another set with MJB_ERR_ARG. ---- */
#define MJB_PRM_BODY_MASS 0
#define MJB_PRM_BODY_INERTIA 1
#define MJB_PRM_DOF_DAMPING 2
#define MJB_PRM_DOF_ARMATURE 3
#define MJB_PRM_ACTUATOR_GEAR 4
#define MJB_PRM_ACTUATOR_GAINPRM 5
#define MJB_PRM_ACTUATOR_BIASPRM 6
#define MJB_PRM_GEOM_FRICTION 7
#define MJB_PRM_GRAVITY 8
#define MJB_PRM_N 9
/* Write the rows of field `name` from src [batch, n] (src_dtype MJB_F32 or MJB_F64; src_on_device = 0: host memory, 1: device memory of
 * the data's device).  env_mask: optional [batch] bytes in device memory, non-zero = write that environment's row; NULL = every row.
 * The first call for a field initialises every row to the model's values, so rows outside the mask keep those.  The copy and the
 * re-derivation of body_subtreemass / pair friction run on the data's stream (a small kernel), behind the launches already queued;
 * host memory is read before the call returns.  MJB_ERR_ARG: unknown name; host values that are not finite; src or env_mask not
 * device memory of the data's device, or the allocation behind it shorter than batch * n elements / batch bytes
 * (hipPointerGetAttributes / hipMemGetAddressRange, as for mjb_rollout_ctrl's table). */
int mjb_set_env_param(mjbData* d, const char* name, const void* src, int src_dtype, int src_on_device, const unsigned char* env_mask);
/* host_out [batch, n] float64: the rows of a batched field, or the model's values broadcast to every environment.  Synchronises. */
int mjb_get_env_param(mjbData* d, const char* name, double* host_out);
/* Return field `name` to the shared model value for every environment (frees its rows after the stream has drained). */
int mjb_clear_env_param(mjbData* d, const char* name);
/* *mask = the batched fields, bit MJB_PRM_* per field. */
int mjb_env_param_mask(mjbData* d, int* mask);
/* mjb_model_kernel_source for a data object whose batched fields are `params_mask` (bits MJB_PRM_*); mask 0 gives the same text. */
long mjb_model_kernel_source_params(mjbModel* m, int kind, int dtype, int lanes, int nconmax, int nefcmax, int params_mask, char* buf, long cap);

/* gains of MJB_CTRL_FEEDBACK, host float64: K [nu, 2nv] row-major, u0 [nu], q0 [nq], v0 [nv] (NULL = zeros); shared by all environments */
int mjb_set_feedback(mjbData* d, const double* K, const double* u0, const double* q0, const double* v0);

/* the same law as a STANDALONE batched kernel for the host-driven loop (one K for many environments: K dx is a GEMM [batch, 2nv] x
 * [2nv, nu], on MFMA in fp32): writes data.ctrl on the device from the current qpos / qvel, then the host calls mjb_step / mjb_step_host.
 * Optional ctrl noise of the reference law (lqr.py:160-165): ctrl += std[a] * table[(step + env * env_stride) mod nsteps][a] before the
 * clip (also inside MJB_CTRL_FEEDBACK rollouts, step = the rollout's step counter); mjb_set_feedback_noise(d, NULL, NULL, 0, 0) switches it off.  Host float64 inputs: std [nu], table [nsteps, nu]. */
int mjb_set_feedback_noise(mjbData* d, const double* noise_std, const double* noise_table, int nsteps, int env_stride);
int mjb_feedback_ctrl(mjbData* d, int step);

/* ---- observations: ObservationExtractor.__call__ with as_dict=False (reference observations.py:98-174) ----
 * flags: bit 0 qpos, 1 qvel, 2 ctrl, 3 sensordata, 4 time, 6 body positions at the inertial frames, 7 (value 128) qacc_warmstart [nv],
 * the solver's warm start after the step - no reference key; it comes LAST in the row, behind the sorted keys, so rows of specs
 * without it are unchanged (the rollout ring of mjb_rollout_ctrl feeds it to mjb_transition_fd_points). */
int mjb_obs_spec_create(mjbData* d, int flags, int nsite, const int* site_ids, int nbody, const int* body_ids,
                        int ngeom, const int* geom_ids, int nsubtree, const int* subtree_ids, mjbObsSpec** out);
void mjb_obs_spec_free(mjbObsSpec* s);
int mjb_obs_dim(const mjbObsSpec* s);
int mjb_obs_gather(mjbData* d, const mjbObsSpec* s, void* out_dev /* [batch, dim], dtype of the data */);

/* the ONE collective of the path: all-gather of the flat observation block over RCCL / xGMI for a host that owns
 * an ncclComm_t (one process per GPU): send_dev [count_per_rank] -> recv_dev [nranks * count_per_rank], dtype MJB_F32 / MJB_F64, on
 * hip_stream.  The Python front uses torch.distributed's all_gather_into_tensor instead (distributed.all_gather_obs); this entry
 * point is the same ncclAllGather for a non-Python host.  The library does not link RCCL: it resolves ncclAllGather from the RCCL
 * already in the process, else from librccl.so.1. */
int mjb_allgather_obs(void* nccl_comm, const void* send_dev, void* recv_dev, long count_per_rank, int dtype, void* hip_stream);

/* ---- mjd_transitionFD (reference linearization.py:16-35): float64 on device.
 * A_host [batch, 2nv, 2nv], B_host [batch, 2nv, nu], row-major ---- */
int mjb_transition_fd(mjbData* d, double eps, int centered, double* A_host, double* B_host);
/* the same without the final host copy: pointers to the library's PINNED result blocks (same layouts), valid until the next
 * mjb_transition_fd* call on this data object — at humanoid batch 512 the two blocks are 16.5 MB */
int mjb_transition_fd_pinned(mjbData* d, double eps, int centered, const double** A_pinned, const double** B_pinned);

/* ---- mjd_transitionFD at caller-chosen points: T x batch (state, control) points held in device memory, linearised in one submission
 * with the results left on the device.  Replaces the reference's linearisation called once per step from a controller loop
 * (mujoco_template/linearization.py:16-35 from runtime.py:631-663) when a whole trajectory is linearised (iLQR, time-varying LQR).
 * Point (t, e), t in [0, T), e in [0, batch), reads x[t * x_step_stride + e * x_env_stride + i] of qpos [nq], qvel [nv], ctrl [nu] and
 * qacc_warmstart [nv] (NULL = zeros at every point): device memory of the data's device in the data's dtype, strides in elements,
 * >= 0 (0 = broadcast), so columns of a rollout ring [T, batch, dim] and a [batch, T, nu] control tensor are read in place.
 * A_dev [T, batch, 2nv, 2nv], B_dev [T, batch, 2nv, nu]: float64 device memory of the caller, row-major, layout and signs of
 * mjb_transition_fd.  Block (t, e) is bit for bit what mjb_transition_fd returns for environment e once the data's qpos, qvel, ctrl and
 * qacc_warmstart rows of e hold point (t, e): e's per-environment parameter rows, the data's current options, the one-sided difference
 * at a ctrlrange bound, every column restarting from the same warm start, the specialised kernel when one is loaded.
 * The data's own state, time and engine flags are not touched.  Everything is enqueued on the data's stream; the call does not
 * synchronise - except when the per-column scratch has to grow (the first call, or more points per slab than any call before): the old
 * block is freed, which waits for the device.  The scratch is one block per data object: after mjb_set_stream to another stream, the
 * next mjb_transition_fd* call makes that stream wait (an event, on the device) for the FD launches still queued on the old one.
 * The points run in slabs whose per-column scratch stays under a fixed budget (MJB_FD_SLAB_BYTES overrides it), slab after
 * slab on the stream; the result does not depend on the slab size.
 * Checked before anything is launched (MJB_ERR_ARG, state and engine flags untouched): T >= 1, T * batch < 2^31, eps > 0, strides >= 0,
 * every array of non-zero width non-NULL (qacc_warmstart excepted), device-accessible memory of the data's device
 * (hipPointerGetAttributes), and the highest element read or written, (T-1)*step_stride + (batch-1)*env_stride + n-1, inside the
 * allocation behind its pointer (hipMemGetAddressRange). */
int mjb_transition_fd_points(mjbData* d, int T, const void* qpos, long qpos_step_stride, long qpos_env_stride,
                             const void* qvel, long qvel_step_stride, long qvel_env_stride,
                             const void* ctrl, long ctrl_step_stride, long ctrl_env_stride,
                             const void* qacc_warmstart, long ws_step_stride, long ws_env_stride,
                             double eps, int centered, double* A_dev, double* B_dev);
/* slabs the last mjb_transition_fd_points on this data object ran in (0: none yet) */
int mjb_fd_points_slabs(const mjbData* d);

/* ---- the sensor half of mjd_transitionFD: C = d sensordata / d[dq; dv], D = d sensordata / d ctrl, with ns = nsensordata rows.
 * The reference passes None, None for them (mujoco_template/linearization.py:28-34); these two calls complete that call site for
 * output-feedback design (observers, Kalman gains, LQG) on the device.  The sensordata differenced is what one step from each
 * perturbed point leaves (mj_step: the sensors of its last forward pass), subtracted as it is - framequat rows get no quaternion
 * treatment - under the rule of (A, B): centred where both nudges are valid, one-sided at a ctrlrange bound, inputs in the order
 * dq | dv | ctrl.  (A, B) are bit for bit those of the calls above; the columns are the same launch, which also keeps every
 * column's sensordata (ns float64 per column of scratch more), and one more small kernel differences them.
 * mjb_transition_fd_sensors: the pinned-view form of mjb_transition_fd_pinned with C [batch, ns, 2nv] and D [batch, ns, nu] beside
 * A and B (same validity, same zero-copy rule for small batches).  A model without sensors: *C_pinned = *D_pinned = NULL.
 * mjb_transition_fd_points_sensors: mjb_transition_fd_points with C_dev [T, batch, ns, 2nv] and D_dev [T, batch, ns, nu], float64
 * device memory of the caller checked like A_dev and B_dev; ns == 0 or nu == 0: nothing is written there and NULL is allowed.
 * Slabs as above, the sensor scratch counted in the budget. ---- */
int mjb_transition_fd_sensors(mjbData* d, double eps, int centered, const double** A_pinned, const double** B_pinned,
                              const double** C_pinned, const double** D_pinned);
int mjb_transition_fd_points_sensors(mjbData* d, int T, const void* qpos, long qpos_step_stride, long qpos_env_stride,
                                     const void* qvel, long qvel_step_stride, long qvel_env_stride,
                                     const void* ctrl, long ctrl_step_stride, long ctrl_env_stride,
                                     const void* qacc_warmstart, long ws_step_stride, long ws_env_stride,
                                     double eps, int centered, double* A_dev, double* B_dev, double* C_dev, double* D_dev);

/* ---- batched LQR / iLQR on the arrays above: the backward (Riccati) recursion and the line search's candidate controls.  The
 * reference designs its controllers from ONE (A, B) with scipy.linalg.solve_discrete_are (examples/humanoid/controllers/lqr.py:114);
 * this is the finite-horizon, time-varying form of that recursion along a trajectory, fed by mjb_transition_fd_points.
 * Everything is float64 DEVICE memory, row-major.  An mjbStrided array holds block (t, e) at ptr + t * step_stride + e * env_stride
 * (strides in elements, >= 0, 0 = broadcast), so the [T, batch, ...] blocks of mjb_transition_fd_points, their permuted
 * [batch, T, ...] views and a constant Q, R passed once (both strides 0) are read in place.  `batch` is the number of trajectories
 * of THIS call - it need not be the data object's batch, which only supplies the device and the stream.
 * Both calls check, before anything is launched (MJB_ERR_ARG with a message, outputs untouched): 1 <= nx <= 64, 1 <= nu <= 32, T >= 1,
 * batch >= 1, strides >= 0, every required pointer non-NULL and device-accessible memory of the data's device
 * (hipPointerGetAttributes), and the highest element read or written inside the allocation behind it (hipMemGetAddressRange).
 * Both are enqueued on the data's stream as ONE kernel launch, use no scratch memory, copy nothing to the host and do not synchronise. */
typedef struct mjbStrided { const double* ptr; long step_stride, env_stride; } mjbStrided;

/* For every trajectory e and t = T-1 .. 0, from Vx = VxT, Vxx = VxxT (the Gauss-Newton form: no second-order dynamics terms):
 *   Qx = lx + A' Vx, Qu = lu + B' Vx, Qxx = lxx + A' Vxx A, Quu = luu + B' Vxx B + mu I, Qux = lux + B' Vxx A,
 *   k = -Quu^-1 Qu, K = -Quu^-1 Qux (Cholesky), dV[0] += k' Qu, dV[1] += k' Quu k / 2,
 *   Vx = Qx + K' Quu k + K' Qu + Qux' k, Vxx = sym(Qxx + K' Quu K + K' Qux + Qux' K).
 * With lx = lu = 0 this is the discrete Riccati recursion and K_t the time-varying LQR gain.
 * A [nx, nx], B [nx, nu], lx [nx], lu [nu], lxx [nx, nx], luu [nu, nu], lux [nu, nx] (ptr NULL = 0) per (t, e); VxT [nx], VxxT [nx, nx]
 * (symmetric), mu [1] per e (step_stride ignored).  Outputs, dense: k [T, batch, nu], K [T, batch, nu, nx], dV [batch, 2],
 * status [batch] int32, and optionally (NULL = not wanted) V0x [batch, nx], V0xx [batch, nx, nx].
 * status[e] = 0, or 1 + t for the first (highest) step t at which the Cholesky of Quu met a pivot that is <= 0 or not finite: that
 * trajectory stops there, its k, K blocks of steps <= t, its dV, V0x, V0xx are written as zeros, the others are unaffected - an
 * ordinary outcome of an iLQR iteration (the caller raises mu), reported through memory and not an error of the call. */
typedef struct mjbLqrBackward {
  int T, batch, nx, nu;
  mjbStrided A, B, lx, lu, lxx, luu, lux;
  mjbStrided VxT, VxxT, mu;
  double *k, *K, *dV, *V0x, *V0xx;
  int* status;
} mjbLqrBackward;
int mjb_lqr_backward(mjbData* d, const mjbLqrBackward* p);

/* Control-limited form of mjb_lqr_backward (control-limited DDP: Tassa, Mansard, Todorov, ICRA 2014) for controls that stay inside a
 * box lo <= u <= hi - the reference clips its LQR law to the model's ctrlrange (examples/humanoid/controllers/lqr.py:147-170), and a
 * backward pass that does not know the limits returns gains that push a saturated actuator further into its bound.
 * `base` is read exactly as mjb_lqr_backward reads it (Qx, Qu, Qxx, Quu, Qux are formed the same way, mu included); u [nu] per (t, e)
 * are the nominal controls; lo / hi [nu] (NULL, or +-inf entries: unbounded on that side; lo <= hi is the caller's duty).  Per step,
 * with lob = lo - u_t, hib = hi - u_t:
 *   1. the QP  min x' Quu x / 2 + Qu' x,  lob <= x <= hib  by projected Newton from x = clip(0, lob, hib): g = Qu + Quu x, clamped set
 *      c = (x == lob & g > 0) | (x == hib & g < 0), Newton target x*_f = -Quu_ff^-1 (Qu_f + Quu_fc x_c), x*_c = x_c (a point, not an
 *      increment).  Inside the box it is taken whole, and the QP ends when the clamped set at x* equals c (tolerance-free, finite);
 *      otherwise an Armijo search (ratio 0.1, factor 0.6) on clip(x + s (x* - x)).  No free control: done.  At most 64 iterations and
 *      64 search trials (compile-time constants: the kernel ends in bounded time on any input); a cap or a failed search keeps the
 *      last iterate;
 *   2. the polish, one solve on the final set: [K | k]_f = -Quu_ff^-1 [Qux_f | Qu_f + Quu_fc x_c], K_c = 0, k_c = the bound itself
 *      (lob or hib as computed), then k = clip(k, lob, hib) - accuracy does not depend on a QP tolerance, and with an empty set the
 *      step is bitwise that of mjb_lqr_backward;
 *   3. the value update and dV of mjb_lqr_backward with this k, K and the full Quu.
 * status[e]: 1 + t for a pivot that is <= 0 or not finite in any factorisation of step t (as mjb_lqr_backward: zeros, the other
 * trajectories untouched), else -(1 + t) for the highest step whose QP hit a cap or whose search failed (results finite and inside
 * the box), else 0.  clamped [T, batch] int32: bit a set when control a is clamped at that step (0 for steps not solved);
 * qp_iters [batch] int32: the largest iteration count of any step.  Checks, launch and stream as mjb_lqr_backward. */
typedef struct mjbLqrBackwardBox {
  mjbLqrBackward base;
  mjbStrided u;
  const double *lo, *hi;
  int *clamped, *qp_iters;
} mjbLqrBackwardBox;
int mjb_lqr_backward_box(mjbData* d, const mjbLqrBackwardBox* p);

/* For every trajectory e and step size alphas[j], from dx = dx0[e] (ptr NULL = 0; step_stride ignored):
 *   c_t = clamp(u_t + alphas[j] k_t + K_t dx, lo, hi),  dx = A_t dx + B_t (c_t - u_t)     for t = 0 .. T-1
 * cand [batch, nalpha, T, nu] dense, float64 or (out_f32 != 0) float32 = the float64 value rounded once - what mjb_rollout_ctrl of a
 * float32 data object takes.  k [nu], K [nu, nx], u [nu] per (t, e): the outputs of mjb_lqr_backward are passed with
 * step_stride = batch * n, env_stride = n.  alphas [nalpha], 1 <= nalpha <= 64; lo / hi [nu], NULL = unbounded on that side. */
typedef struct mjbLqrCandidates {
  int T, batch, nx, nu, nalpha, out_f32;
  mjbStrided A, B, k, K, u, dx0;
  const double *alphas, *lo, *hi;
  void* cand;
} mjbLqrCandidates;
int mjb_lqr_candidates(mjbData* d, const mjbLqrCandidates* p);

/* c [M, N] = a' b for a [K, M], b [K, N] (device float64, dense, M, N <= 64, K >= 1) through the tile product of the two kernels
 * above alone: a diagnostic that pins the operand and result fragment maps of v_mfma_f64_16x16x4_f64 with exact integer data. */
int mjb_lqr_gemm_tn(mjbData* d, int M, int N, int K, const double* a, const double* b, double* c);

/* ---- infinite-horizon LQR design for a batch of systems: the stabilising solution X of the discrete algebraic Riccati equation
 *   A' X A - X - A' X B (R + B' X B)^-1 B' X A + Q = 0     and the gain     K = (R + B' X B)^-1 B' X A.
 * The reference designs each of its controllers this way, one system at a time on the host, with scipy.linalg.solve_discrete_are
 * (examples/humanoid/controllers/lqr.py:114, examples/drone/controllers/lqr.py:358-369); with per-environment model parameters every
 * environment has its own (A, B) (mjb_transition_fd_points), and this call designs all of them on the device.
 * The structure-preserving doubling algorithm, per problem e in float64 (iteration k holds 2^k steps of the Riccati recursion):
 *   R = L L' (Cholesky),  G_0 = sym(B R^-1 B'),  H_0 = Q,  A_0 = A
 *   repeat k = 0, 1, ...:
 *     W = I + G_k H_k;  LU of W with partial pivoting, the pivot row the LOWEST index among the rows of largest |.|
 *     X_A = W^-1 A_k,  X_G = W^-1 G_k
 *     H_{k+1} = sym(H_k + A_k' (H_k X_A)),  G_{k+1} = sym(G_k + A_k X_G A_k'),  A_{k+1} = A_k X_A
 *     change = max|H_{k+1} - H_k| / max|H_{k+1}|
 *   until change <= tol or k + 1 == max_iter        (on change alone, never on stagnation: change may rise before it collapses)
 *   X = H (bitwise symmetric),  K = (R + B' X B)^-1 B' X A (Cholesky).
 * SIGN: K is the gain of the reference and of mjb_set_feedback (u = u0 - K dx) - the NEGATIVE of the K of mjb_lqr_backward.
 * Q [nx, nx] and R [nu, nu] are taken as symmetric and not checked: only their LOWER triangles are read.  No cross term N.
 * A [nx, nx], B [nx, nu], Q, R per problem e at ptr + e * env_stride (step_stride ignored; env_stride 0 = shared by all problems).
 * Outputs, dense: X [batch, nx, nx], K [batch, nu, nx], iters [batch] int32, status [batch] int32, change [batch] (NULL = not wanted).
 * status[e]: 0 converged; 1 a Cholesky pivot of R or of R + B' X B was <= 0 or not finite; 2 an LU pivot was zero or not finite, or
 * an iterate was not finite (a system that is not stabilisable ends this way); 3 max_iter iterations without change <= tol.  For a
 * non-zero status X[e] and K[e] are written as ZEROS, iters[e] and change[e] hold what was reached (change = +inf when not finite),
 * and no other problem is affected.  A problem's results are bitwise the same at any position of any batch.
 * 1 <= max_iter <= 64 and tol >= 0: the kernel ends in bounded time on any input.  `batch` is this call's, not the data object's.
 * Checks (before anything is launched: MJB_ERR_ARG with a message, outputs untouched), launch and stream as mjb_lqr_backward: sizes,
 * tol, max_iter, strides >= 0, required pointers, device memory of the data's device, the highest element inside its allocation; ONE
 * kernel launch on the data's stream (one workgroup per problem, everything resident in LDS), no scratch memory, no host copy, no
 * synchronisation. */
typedef struct mjbLqrDare {
  int batch, nx, nu, max_iter;
  double tol;
  mjbStrided A, B, Q, R;
  double *X, *K, *change;
  int *iters, *status;
} mjbLqrDare;
int mjb_lqr_dare(mjbData* d, const mjbLqrDare* p);

/* ---- the poles of a batch of (closed-loop) systems: every eigenvalue of M = A + feedback_sign * B K and rho = max |lambda|.
 * The reference's next line after every design is np.max(np.abs(np.linalg.eigvals(A - B @ K))): it refuses or rescales a gain whose
 * closed-loop spectral radius is not below 1 (examples/drone/controllers/lqr.py:134-137, examples/drone2/main.py:317-318).  With
 * per-environment (A, B) this answers on the device which environments a gain stabilises (rho < 1) and by what margin.
 * SIGN: feedback_sign = -1 is the convention of mjb_lqr_dare and mjb_set_feedback (u = u0 - K dx), +1 that of mjb_lqr_backward.  The
 * sign is applied to K exactly, so (+1, -K) is bitwise (-1, K).  B.ptr and K.ptr both NULL: M = A (open-loop poles; nu is ignored);
 * exactly one of them NULL is an error.
 * The method is LAPACK's for eigenvalues only, per problem e in float64, every iterate resident in LDS, one wavefront per problem:
 *   1. M = A + s B K on the f64 MFMA.  An entry of M that is not finite (as any such entry of A, B or K makes one) ends with status 1.
 *   2. if balance != 0: Parlett-Reinsch scaling alone (no permutation), radix 2 and therefore exact: dgebal's loop on the 1-norms of
 *      the off-diagonal parts of row and column i with its 0.95 acceptance factor, rows in index order until a full pass changes
 *      nothing, a zero row or column norm leaving that index alone.  scale = D (powers of two); the spectrum computed is that of
 *      D^-1 M D.  balance == 0: scale is all ones.
 *   3. Householder reduction to upper Hessenberg form (a reflector of zero norm is the identity).
 *   4. Francis implicit double-shift QR on the active block alone (dlahqr without Schur vectors): its two-stage small-subdiagonal
 *      deflation test, exceptional shifts at every 10th and 20th sweep since the last deflation, final 2 x 2 blocks standardised as
 *      dlanv2 does.  max_sweeps caps the TOTAL number of sweeps of a problem: 0 = LAPACK's 30 * max(10, nx), else 1 .. that number.
 *   5. the eigenvalues sorted by descending modulus, ties by descending real part, then descending imaginary part.
 * Inputs: A [nx, nx], B [nx, nu], K [nu, nx] per problem e at ptr + e * env_stride (step_stride ignored; env_stride 0 = shared by all
 * problems: one K against per-environment A, B is the robustness sweep).  nx <= 64, nu <= 32.
 * Outputs, dense, all written for every problem: wr, wi [batch, nx] the real and imaginary parts in the order above, a complex pair
 * as exact conjugates (equal wr, wi bitwise negated, the positive one first); rho [batch] = the modulus of the first, the correctly
 * rounded sqrt(wr^2 + wi^2); scale [batch, nx]; sweeps [batch] int32 Francis sweeps done; status [batch] int32: 0 ok, 1 an entry not
 * finite, 2 max_sweeps reached before every eigenvalue had deflated.  For a non-zero status wr[e], wi[e] are NaN and rho[e] is +inf,
 * so that rho < 1 is false for a failed problem (deliberately not the zeros of mjb_lqr_dare, which would read as stable); no other
 * problem is affected.  A problem's results are bitwise the same at any position of any batch.
 * Checks, launch and stream as mjb_lqr_dare (MJB_ERR_ARG with a message before anything is launched, outputs untouched): sizes,
 * feedback_sign, max_sweeps, strides >= 0, required pointers, device memory of the data's device, the highest element inside its
 * allocation; ONE kernel launch on the data's stream, no scratch memory, no host copy, no synchronisation. */
typedef struct mjbLqrEig {
  int batch, nx, nu, feedback_sign, balance, max_sweeps;
  mjbStrided A, B, K;
  double *wr, *wi, *rho, *scale;
  int *sweeps, *status;
} mjbLqrEig;
int mjb_lqr_eig(mjbData* d, const mjbLqrEig* p);

/* ---- the infinite-horizon quadratic cost of running a gain on a batch of systems: the solution P of the discrete Lyapunov equation
 *   P = M' P M + Q + K' R K,     M = A + feedback_sign * B K,     and     J = x0' P x0,
 * the cost of u = u0 - K dx run for ever on (A, B).  For the optimal gain P is the X of mjb_lqr_dare - the P the reference's
 * _solve_lqr_gains hands back beside K (examples/drone/controllers/lqr.py:350-360); for any other gain (a nominal one against every
 * randomised (A_e, B_e), a hand-tuned one, the gain of a cheaper Q) it is scipy.linalg.solve_discrete_lyapunov, one system at a time on
 * the host.  M is the closed loop whose spectral radius the reference checks (examples/drone/controllers/lqr.py:133-137, mjb_lqr_eig):
 * that call answers "is it stable?", this one "what does it cost?".  With transpose != 0 the same iteration solves the Gramian form
 * P = M P M' + S (S = B B' passed as Q: the controllability Gramian, the H2 norm).
 * Squared Smith (doubling) iteration, per problem e in float64 (iterate k holds 2^k steps of the cost sum):
 *   1. M = A + s B K, s = feedback_sign: -1 the convention of mjb_lqr_dare and mjb_set_feedback, +1 that of mjb_lqr_backward.  The sign
 *      is applied to K exactly, so (+1, -K) is bitwise (-1, K).  B.ptr and K.ptr both NULL: M = A (nu is ignored); exactly one of them
 *      NULL is an error.
 *   2. S = sym(Q + K' (R K)).  R.ptr NULL, or no K: S = sym(Q); R without K is an error.  Q [nx, nx] and R [nu, nu] are taken as
 *      symmetric and not checked: only their LOWER triangles are read.  An entry of M or S that is not finite ends with status 1.
 *   3. P_0 = S, M_0 = M;  repeat k = 0, 1, ...:
 *        T = M_k' (P_k M_k)                  (transpose != 0: T = M_k (P_k M_k'))
 *        P_{k+1} = sym(P_k + T),  M_{k+1} = M_k M_k
 *        change = max|P_{k+1} - P_k| / max|P_{k+1}|  (0 / 0 = 0);  iters += 1
 *        an iterate that is not finite ends with status 2 (a closed loop with rho > 1 ends this way: M^(2^k) overflows);
 *        the FIRST change <= tol ends with status 0;  iters == max_iter ends with status 3 (rho == 1 with a marginal mode S sees).
 *      The stop is on change alone and at its first crossing, never on stagnation: with marginal modes that S does not see, change
 *      collapses and then doubles with every further iteration.
 *   4. P = P_k (bitwise symmetric);  with x0: J[e] = sum_i x0_i (P x0)_i, the row sums and the outer sum in index order.
 * Inputs: A [nx, nx], B [nx, nu], K [nu, nx], Q [nx, nx], R [nu, nu], x0 [nx] per problem e at ptr + e * env_stride (step_stride
 * ignored; env_stride 0 = shared by all problems: one K, Q, R against per-environment A, B is the robustness sweep, read without a
 * copy).  nx <= 64, nu <= 32, 1 <= max_iter <= 64, tol >= 0: the kernel ends in bounded time on any input.
 * Outputs, dense: P [batch, nx, nx]; J [batch], required exactly when x0.ptr is given; iters [batch] int32, status [batch] int32,
 * change [batch] (NULL = not wanted).  For a non-zero status P[e] is NaN and J[e] is +inf, so that J < bound is false for a failed
 * problem (the convention of mjb_lqr_eig, deliberately not the zeros of mjb_lqr_dare); iters[e] and change[e] hold what was reached
 * (change = +inf when not finite); no other problem is affected.  A problem's results are bitwise the same at any position of any batch.
 * Checks, launch and stream as mjb_lqr_dare / mjb_lqr_eig (MJB_ERR_ARG with a message before anything is launched, outputs
 * untouched): sizes, feedback_sign, tol, max_iter, strides >= 0, required pointers, device memory of the data's device, the highest
 * element inside its allocation; ONE kernel launch on the data's stream (one workgroup per problem, everything resident in LDS, the
 * products on the f64 MFMA), no scratch memory, no host copy, no synchronisation. */
typedef struct mjbLqrDlyap {
  int batch, nx, nu, feedback_sign, transpose, max_iter;
  double tol;
  mjbStrided A, B, K, Q, R, x0;
  double *P, *J, *change;
  int *iters, *status;
} mjbLqrDlyap;
int mjb_lqr_dlyap(mjbData* d, const mjbLqrDlyap* p);

/* ---- the quadratic trajectory cost, its first-order expansion and the choice among candidates: what an iLQR iteration or a sampling
 * planner needs between mjb_rollout_ctrl / mjb_transition_fd_points and mjb_lqr_backward / mjb_lqr_candidates, on the device.  The
 * reference's humanoid controller builds its Q in the 2nv tangent space (examples/humanoid/controllers/lqr.py:97-114) and takes the
 * state difference with mj_differentiatePos (examples/humanoid/controllers/lqr.py:153); this is that cost along whole trajectories.
 *
 * A trajectory e has T + 1 points: x_0 the start state, x_{t+1} the state after step t.  For point t, in float64, inputs widened exactly:
 *   dx_t = [ differentiatePos(qref_t -> qpos_t, dt = 1) ; qvel_t - vref_t ]     (2nv; sign and quaternion rule of
 *                                                                                 mjb_differentiate_pos(qvel_out, 1, qref, qpos))
 *   du_t = u_t - uref_t
 *   cost_t[e, t] = dx_t' Q_t dx_t / 2 + du_t' R_t du_t / 2    (t < T),     cost_t[e, T] = dx_T' Qf dx_T / 2
 *   cost[e] = sum_t cost_t[e, t]; a sum that is NaN or infinite is stored as +inf (cost is never NaN)
 *   lx[t, e] = Q_t dx_t, lu[t, e] = R_t du_t (t < T), VxT[e] = Qf dx_T   - what mjb_lqr_backward takes (lxx = Q, luu = R, VxxT = Qf are
 *   the caller's own arrays).  Q, R, Qf are TAKEN AS SYMMETRIC, not checked: the kernel reads Q[j, i] for Q[i, j].
 * Inputs, all (ptr, step_stride, env_stride) arrays as above (strides in elements, >= 0, 0 = broadcast):
 *   qpos0 [nq], qvel0 [nv] per e (step_stride ignored); qpos [nq], qvel [nv] per (t, e), t = 0 .. T-1: the state AFTER step t - two
 *   pointers, so the columns of a rollout ring [T, batch, dim] are read in place; ctrl [nu] per (t, e).  These carry a dtype (MJB_F32 /
 *   MJB_F64): the four state arrays must agree, the control has its own.
 *   float64: qref [nq] (required - a zero quaternion is no default), vref [nv] (NULL = 0) per point t = 0 .. T; uref [nu] (NULL = 0),
 *   Q [2nv, 2nv], R [nu, nu] per (t, e), t < T; Qf [2nv, 2nv] per e (step_stride ignored).
 * nq, nv, nu and the joint table are the data object's model; nv <= 64, 1 <= nu <= 64, T >= 1, batch >= 1 (the call's own, not the data's).
 * Outputs, dense float64: cost [batch], cost_t [batch, T + 1] (required: it is also the staging of the sum), and optionally
 * (NULL = not wanted) lx [T, batch, 2nv], lu [T, batch, nu], VxT [batch, 2nv].
 * Two kernel launches on the data's stream; no scratch, no allocation, no host copy, no synchronisation, no atomics.  cost_t and the
 * gradient blocks of a point depend on that point's inputs and (nv, nu) alone and cost[e] is summed in an order fixed by T, so a
 * trajectory gives bitwise the same results at any position of any batch.
 * Checked before anything is launched (MJB_ERR_ARG with a message, outputs untouched): the sizes, strides >= 0, required pointers,
 * device memory of the data's device (hipPointerGetAttributes), the highest element read or written inside the allocation behind
 * each pointer (hipMemGetAddressRange). */
typedef struct mjbStridedIn { const void* ptr; long step_stride, env_stride; int dtype; } mjbStridedIn;
typedef struct mjbTrajCost {
  int T, batch;
  mjbStridedIn qpos0, qvel0, qpos, qvel, ctrl;
  mjbStrided qref, vref, uref, Q, R, Qf;
  double *cost, *cost_t, *lx, *lu, *VxT;
} mjbTrajCost;
int mjb_traj_cost(mjbData* d, const mjbTrajCost* p);

/* nprob problems with ncand candidates each: cost [nprob, ncand] float64, cand [nprob, ncand, T, nu] dense in cand_dtype (what
 * mjb_lqr_candidates writes; for a sampling planner the control tensor itself with nprob = 1), u_out [nprob, T, nu] in out_dtype.
 * 1 <= ncand <= 2^20, nprob >= 1, T * nu <= 2^22.  best [nprob] int32, best_cost [nprob], weights [nprob, ncand]: NULL = not wanted.
 * MJB_SELECT_ARGMIN: best[g] = the lowest index among the candidates of minimal FINITE cost, best_cost[g] its cost,
 *   u_out[g] = cand[g, best] (equal dtypes: a bit copy; float64 -> float32 rounded once; float32 -> float64 exact).  No finite cost:
 *   best = -1, best_cost = +inf and u_out[g] is NOT written - pass the nominal as u_out and it is kept.
 * MJB_SELECT_SOFTMIN (the MPPI update): w_j = exp(-(c_j - c_min) / temperature) over the finite costs, 0 for the others, normalised
 *   to sum 1; u_out[g] = sum_j w_j cand[g, j] in float64, rounded once on output; best / best_cost as above; weights the w_j
 *   (zeros when no cost is finite, u_out then not written).  temperature > 0 is checked.
 * One launch on the data's stream, no allocation, no synchronisation, deterministic.  Checks as for mjb_traj_cost. */
#define MJB_SELECT_ARGMIN 0
#define MJB_SELECT_SOFTMIN 1
typedef struct mjbTrajSelect {
  int nprob, ncand, T, nu, mode, cand_dtype, out_dtype;
  double temperature;
  const double* cost;
  const void* cand;
  void* u_out;
  int* best;
  double *best_cost, *weights;
} mjbTrajSelect;
int mjb_traj_select(mjbData* d, const mjbTrajSelect* p);

/* ---- the equilibrium controls of a batch of operating points: the minimum-norm u of
 *   min_u | u @ moment - qfrc |_2,     moment [nu, nv] the actuator moment matrix,  qfrc [nv] the force inverse dynamics asks for,
 * with the singular values of moment and a conditioning verdict per problem.  It is the head of the reference's controller design,
 * ctrl0 = qfrc0 @ pinv(actuator_moment) behind an SVD guard against a singular moment matrix (mujoco_template/setpoints.py:50-51,
 * examples/humanoid/controllers/lqr.py:83): ctrl0 is both the point mjb_transition_fd_points linearises at and the u0 of the feedback
 * law.  mjb_inverse leaves qfrc_inverse [batch, nv] and actuator_moment [batch, nu, nv] in device memory; this call reads them there.
 * One-sided (Hestenes) Jacobi SVD of G = moment' itself - never an eigen-solve of G'G, which would square the condition number the
 * guard tests; Jacobi also keeps high relative accuracy when actuator rows differ by orders of magnitude (gear ratios).  Per problem
 * e, in float64, float32 inputs widened exactly:
 *   1. G [nv, nu], column a = row a of moment; V = I [nu, nu].  An entry of moment or qfrc that is not finite ends with status 1, and so
 *      does a float64 sum(G^2) that is not finite (finite entries above 1e154, whose squares overflow: no norm can be formed).
 *   2. tol = 2^-52, floor = tol^2 * sum(G^2): a column whose squared norm is <= floor is rounding noise and is never rotated (without
 *      this nu > nv never converges).
 *   3. Sweeps of a fixed round-robin schedule: n' = nu rounded up to even, n' - 1 rounds of n' / 2 disjoint pairs (round rd: pair 0 =
 *      (n' - 1, rd), pair k = ((rd + k) mod (n' - 1), (rd - k) mod (n' - 1)); a pair with an index >= nu is idle); the pairs of a
 *      round run concurrently.  For a pair i < j: a = |g_i|^2, b = |g_j|^2, c = g_i . g_j; skipped if c == 0 or
 *      |c| <= tol sqrt(a) sqrt(b) or min(a, b) <= floor; otherwise z = (b - a) / (2 c), t = sign(z) / (|z| + hypot(1, z)) (z == 0:
 *      t = 1), cs = 1 / sqrt(1 + t^2), sn = cs t, (g_i, g_j) <- (cs g_i - sn g_j, sn g_i + cs g_j) and the same for V.
 *   4. A sweep without a rotation ends the iteration (it counts in sweeps); max_sweeps sweeps that each rotated something end with
 *      status 2.  max_sweeps: 0 = the default of 30, else 1 .. 64.
 *   5. sigma_j = sqrt(|g_j|^2), sorted descending, ties by lower index; r = min(nu, nv); sv = the first r; rcond = sigma_r / sigma_1
 *      (0 when sigma_1 == 0); rank = the count of sigma_j > rcond_min * sigma_1 among them; rcond < rcond_min ends with status 3 - the
 *      reference's TemplateError("... singular or ill-conditioned"), reported per environment instead of raised.
 *   6. ctrl = sum_j v_j (g_j . qfrc) / sigma_j^2 over the first r columns in sorted order (terms with sigma_j == 0 skipped);
 *      residual = max_i |(ctrl @ moment - qfrc)_i|, moment re-read from global memory: the force no actuator can supply (a free root);
 *      pinv [nv, nu] = sum_j g_j v_j' / sigma_j^2, the shape and meaning of numpy.linalg.pinv(moment).  Every reduction runs in a fixed order.
 * Inputs: moment [nu, nv], qfrc [nv] per problem e at ptr + e * env_stride (step_stride ignored; env_stride 0 = shared by all
 * problems), MJB_F32 or MJB_F64 each.  1 <= nu <= 32, 1 <= nv <= 64; batch is the call's own, not the data object's; rcond_min >= 0 and
 * finite (the reference's guard is 1e-12).
 * Outputs, dense: ctrl [batch, nu], sv [batch, min(nu, nv)], rcond [batch], residual [batch], pinv [batch, nv, nu] (NULL = not
 * wanted); rank, sweeps, status [batch] int32.  For a non-zero status ctrl[e] and pinv[e] are NaN and residual[e] is +inf (the
 * convention of mjb_lqr_eig / mjb_lqr_dlyap: a failed set-point cannot be applied silently); sv, rcond, rank and sweeps hold what was
 * reached (status 1: NaN, NaN, 0, 0); no other problem is affected.  A problem's results are bitwise the same at any position of any batch.
 * Checks, launch and stream as mjb_lqr_dlyap (MJB_ERR_ARG with a message before anything is launched, outputs untouched): sizes,
 * rcond_min, strides >= 0, required pointers, device memory of the data's device, the highest element inside its allocation; ONE
 * kernel launch on the data's stream (one wavefront per problem, G and V resident in LDS), no scratch memory, no allocation, no host
 * copy, no synchronisation. */
typedef struct mjbSetpoint {
  int batch, nu, nv, max_sweeps;
  double rcond_min;
  mjbStridedIn moment, qfrc;
  double *ctrl, *sv, *rcond, *residual, *pinv;
  int *rank, *sweeps, *status;
} mjbSetpoint;
int mjb_setpoint_ctrl(mjbData* d, const mjbSetpoint* p);

/* ---- the linear feedback law from device tensors: per-environment and time-varying gains.  It is the law of the reference's LQR
 * controllers (examples/humanoid/controllers/lqr.py:147-170, examples/drone/controllers/lqr.py:220-278: mj_differentiatePos against the
 * goal, ctrl0 - K dx, clip to ctrlrange) with K, u0, q0, v0 read where mjb_setpoint_ctrl, mjb_lqr_dare and mjb_lqr_backward left them:
 * device memory, one block per environment and / or per step.  mjb_set_feedback / MJB_CTRL_FEEDBACK / mjb_feedback_ctrl keep their one
 * host-supplied law shared by all environments and are not involved.
 * For environment e of the data object at step index t, all arithmetic in float64, float32 inputs widened exactly:
 *   dx  = [ differentiatePos(q0 -> qpos_e, dt = 1) ; qvel_e - v0 ]      # 2nv
 *   s_a = sum_k K[a, k] dx[k]
 *   u_a = u0[a] + feedback_sign * s_a
 *   if clip and actuator a is ctrl-limited: u_a = min(max(u_a, lo_a), hi_a)
 *   ctrl_e[a] = u_a                                                     # rounded once to the data's dtype
 * The sign and quaternion rule of dx are those of mjb_differentiate_pos(qvel_out, 1, q0, qpos).  Every product K[a, k] dx[k] is rounded
 * once and row a is added in the order k = 0 .. 2nv - 1.
 * Inputs: K [nu, 2nv] row-major, u0 [nu], q0 [nq], v0 [nv] (v0.ptr NULL = zeros), each an mjbStridedIn: the block of (t, e) sits at
 * ptr + t * step_stride + e * env_stride (strides in elements, >= 0, 0 = broadcast), MJB_F32 or MJB_F64 per array.  Strides (0, 0): a
 * shared law; (0, n): per environment (domain-randomised LQR); (n, 0): time-varying (TVLQR tracking); both: per environment and step
 * (the closed-loop forward pass of iLQR with u0 = ubar + alpha k, q0 / v0 the nominal state, feedback_sign = +1).  qpos, qvel and ctrl
 * are the data object's own arrays; nq, nv, nu, the joint table and actuator_ctrllimited / actuator_ctrlrange its model's.
 * nv <= 64, 1 <= nu <= 32 (the limits of mjb_lqr_dare).
 * feedback_sign: -1 is the convention of mjb_lqr_dare and mjb_set_feedback (u = u0 - K dx), +1 that of mjb_lqr_backward; anything else
 * is MJB_ERR_ARG.  clip = 0 leaves u_a unclipped.
 * env_mask: optional [batch] bytes in device memory; a zero entry = that environment's ctrl, status and record row are not written
 * (the bytes of mjb_lqr_dare's status == 0 feed it directly).
 * status: optional [batch] int32 in device memory; bits are ORed in, so it is sticky over the steps of a rollout (the caller zeroes it).
 *   bit 0 (1): a value of this environment's K, u0, q0, v0, qpos or qvel, or a resulting u_a, was not finite.  That step's ctrl is then
 *              written as ZEROS for the whole environment (what MuJoCo does with a bad ctrl): a failed design cannot be applied silently.
 *   bit 1 (2): at least one actuator was clipped (not reported for a step that raised bit 0).
 * u_rec: optional record in the data's dtype; the ctrl row just written is also stored at u_rec + t * u_rec_step_stride +
 *   e * u_rec_env_stride - the control tensor of the closed-loop trajectory, [batch, T, nu] as mjb_rollout_ctrl and mjb_lqr_backward take it.
 * One wavefront owns an environment: status is a plain load, OR and store, without atomics, and an environment's ctrl is bitwise the
 * same at any position of any batch, for any batch size, alignment of its K block and layout of the inputs.
 *
 * mjb_feedback_law: ONE launch on the data's stream; writes ctrl for step index t.  No scratch memory, no allocation, no host copy, no
 * synchronisation.
 * mjb_rollout_feedback: for t = 0 .. nstep-1 it enqueues, in order, (1) the law kernel for t, (2) exactly what mjb_step(d, 1) enqueues,
 * (3) when spec != NULL and (t + 1) % obs_every == 0, what mjb_obs_gather enqueues, into row t / obs_every of obs_out_dev
 * [nstep / obs_every, batch, dim]: a ring row holds what the ring of mjb_rollout_ctrl holds for the same controls.  Everything is
 * stream-ordered; no synchronisation and no host read between steps.
 * Checked before anything is launched (MJB_ERR_ARG with a message; state, ctrl and engine flags untouched): the sizes, feedback_sign,
 * nstep >= 1, t >= 0, strides >= 0, the required pointers (K, u0, q0), every pointer device memory of the data's device
 * (hipPointerGetAttributes), and the highest element read or written inside the allocation behind it (hipMemGetAddressRange) - for
 * the rollout with t = nstep-1; u_rec, status, env_mask and the ring included. */
typedef struct mjbFeedbackLaw {
  mjbStridedIn K, u0, q0, v0;
  int feedback_sign, clip;
  const unsigned char* env_mask;
  int* status;
  void* u_rec; long u_rec_step_stride, u_rec_env_stride;
} mjbFeedbackLaw;
int mjb_feedback_law(mjbData* d, const mjbFeedbackLaw* p, int t);
int mjb_rollout_feedback(mjbData* d, const mjbFeedbackLaw* p, int nstep,
                         const mjbObsSpec* spec, void* obs_out_dev, int obs_every);

/* ---- mj_jacSite / mj_jacBody / mj_jacBodyCom / mj_jacSubtreeCom (reference jacobians.py:44-79).
 * kinds[i]: 0 site, 1 body, 2 bodycom, 3 subtreecom.  jacp/jacr host [batch, nreq, 3, nv] float64 (jacr may be NULL) ---- */
int mjb_jac(mjbData* d, int nreq, const int* kinds, const int* ids, double* jacp_host, double* jacr_host);

/* per-phase dumps of the last mjb_forward for parity tests: name in
 * qM qfrc_bias qfrc_passive qfrc_actuator qacc_smooth qfrc_constraint efc_J efc_aref efc_D efc_pos efc_force con cdof cinert cvel (float64 out)
 * and efc_type (int32 out).  Call mjb_debug_forward() first. */
/* diagnostic build (-DMJB_PROFILE) only: per-phase shader-cycle sums since the last call, host_out[24]; zeros otherwise */
int mjb_profile_get(mjbData* d, unsigned long long* host_out);
/* How the last stepping launch (mjb_step / mjb_rollout / mjb_step_host) mapped work to workgroups: out6 = { steps of the launch,
 * environment blocks, resident workgroup slots of the step kernel on this device (0 = unknown), chunk_steps (0 = static map: one
 * workgroup per block for all steps; > 0 = the resident workgroups drew (block, chunk) tickets), fair_bit (0 = hardware age order), 1 if the launch used two wavefronts per environment (small batches) }.
 * The engine picks the map itself (more blocks than slots -> tickets); MJB_CHUNK_STEPS / MJB_FAIR_BIT override it for experiments. */
int mjb_step_schedule(mjbData* d, int* out6);
/* diagnostic kernel (-DMJB_TIMELINE) only: per environment [start, end] of its wave in the last launch (100 MHz clock), HW_ID, XCC_ID */
int mjb_profile_env_get(mjbData* d, unsigned long long* host_out /* [batch, 4] */);
int mjb_debug_forward(mjbData* d);
int mjb_debug_get(mjbData* d, const char* name, void* host_out, long capacity_elems);

#ifdef __cplusplus
}
#endif
#endif
