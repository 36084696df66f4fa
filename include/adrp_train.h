/* adrp_train.h — the training-loop additions to the C-ABI of include/adrp.h, which includes this file at
 * its end (include adrp.h, not this file).  They are additive: ADRP_ABI_VERSION stays 2, and no struct or
 * signature of adrp.h changes.  Kept in a header of their own because tests/test_ppo_abi.py and
 * tests/test_roster_abi.py pin the exact set of adrp_ppo_* / adrp_race_roster_* declarations of adrp.h itself;
 * tests/test_ppo_target_kl_abi.py and tests/test_roster_end_on_abi.py pin this file's the same way. */
#ifndef ADRP_TRAIN_H
#define ADRP_TRAIN_H

#ifndef ADRP_H
#error "include adrp.h, which includes adrp_train.h"
#endif

/* ---------------------------------------------------------------------------------------
 * PPO: target_kl as a device latch, and rate setters for schedules (csrc/ppo_kernel.h, csrc/ppo.hip).
 *
 * SB3 2.3.2 PPO.train(): per minibatch approx_kl_div = mean((exp(log_ratio) - 1) - log_ratio) is recorded, and
 * `if target_kl is not None and approx_kl_div > 1.5 * target_kl` the optimizer step of that minibatch is
 * skipped and both the minibatch and the epoch loop end.  Here the stop is a latch in the learner's device
 * memory, two int32 words:
 *   stop[0]  1 once the stop has tripped
 *   stop[1]  the optimizer steps applied since the last adrp_ppo_train_begin; at a trip, the flat index of
 *            the tripping minibatch
 * The reduce launch of adrp_ppo_update compares its float32 approx_kl, widened to double, with the double
 * product 1.5 * target_kl (a NaN does not trip).  On a trip the five statistics of that minibatch are written,
 * and its Adam launch, which sees the latch set by the launch before it, skips the step: the parameters, Adam's
 * m, v, t and the policy's fragment blobs keep their bits.  Every launch of every later adrp_ppo_update returns
 * at entry and leaves stats_out untouched.  Every read of the latch is of a word that an earlier launch wrote
 * (a kernel boundary), there are no atomics and no host read: the calls stay capturable.  A tripped latch holds
 * until adrp_ppo_train_begin, whatever adrp_ppo_set_target_kl is given afterwards.
 *
 * adrp_ppo_set_target_kl: < 0 turns the stop off (the state after adrp_ppo_create), >= 0 turns it on.
 * adrp_ppo_set_rates: learning_rate > 0, clip_range >= 0 (adrp_ppo_create's validation), clip_range_vf < 0:
 * none.  Host only; it takes effect for the adrp_ppo_update calls made afterwards.  The rates and the target
 * travel by value with each launch, so a captured graph keeps the values it was captured with.
 * adrp_ppo_train_begin clears the latch on `stream`.
 * adrp_ppo_stop_state copies the two words to out_dev2 (device, 2 int32) on `stream`.
 *
 * Refused with ADRP_ERR_INVALID before any device call, through adrp_last_error(NULL): a NULL handle, a NULL
 * out_dev2, a NaN target_kl, invalid rates (a NaN clip_range_vf included).
 * --------------------------------------------------------------------------------------- */
int adrp_ppo_set_target_kl(adrp_ppo_t* ppo, double target_kl);
int adrp_ppo_set_rates(adrp_ppo_t* ppo, double learning_rate, double clip_range, double clip_range_vf);
int adrp_ppo_train_begin(adrp_ppo_t* ppo, void* stream);
int adrp_ppo_stop_state(adrp_ppo_t* ppo, int32_t* out_dev2, void* stream);

/* ---------------------------------------------------------------------------------------
 * Race rosters: the reset mask of a collector that ends an env with its last learner (csrc/roster_kernel.h).
 *
 * adrp_race_roster_done: after adrp_race_roster_step(_env) on the same stream (it reads the alive that launch
 * wrote).  One lane per env, 256-lane blocks: mask_out[e] (uint8 [E]) = 1 where term[e] | trunc[e], or where no
 * learner drone of env e has alive[e * N + d(l)] != 0; else 0.  The alive of the slots that are no learner's is
 * not read, and nothing but mask_out is written.  Refused before any device call: what adrp_race_roster_step
 * refuses of io and agents, and a NULL term, trunc or mask_out.
 * --------------------------------------------------------------------------------------- */
int adrp_race_roster_done(const adrp_race_roster_io* io, const adrp_race_agents_io* agents, const uint8_t* term,
                          const uint8_t* trunc, uint8_t* mask_out, void* stream);

#endif /* ADRP_TRAIN_H */
