// A whole PPO iteration from plain C/C++ through include/acas2d.h -- no Python, no torch.
//
// training_main.py:44-52 (`PPO('MlpPolicy', env).learn()`) on E envs, every step a call of the C ABI:
//   acas2d_reset_f32        the first observation
//   acas2d_collect_f32      T steps of actor, critic, Gaussian sampling and env step in one launch
//   acas2d_gae_f32          the critic's value of the last observation (inside the kernel) and GAE in one launch
//   acas2d_ppo_update_f32   one minibatch update in two launches, over host-shuffled minibatches
// for a few iterations.  The host keeps the parameters in torch's layouts ([out][in], what the update takes) and hands
// the collector and the GAE kernel transposed copies of the first two layers of each net, remade after every iteration.
//
// Everything random on the host comes from ONE 64-bit LCG so that tests/test_gae_kernel.py can restate it:
//   state <- state * 6364136223846793005 + 1442695040888963407   (mod 2^64), starting from 13
//   a weight    = ((state >> 40) / 2^24 - 0.5) * scale           the 13 tensors in the update's order (actor w1 b1 w2 b2 w3
//                 b3, critic likewise, log_std), row-major, scale 0.5 / 0.25 for the two hidden layers' weights, 2^-6 for
//                 the actor's head and 0.125 for the critic's; biases and log_std are 0 and draw nothing
//   a shuffle   = Fisher-Yates from the top: for i = n-1 .. 1: j = (state >> 33) % (i + 1) after one LCG step; swap
// Hyper-parameters: gamma 0.99, lambda 0.95 (gamma x lambda rounded once from double), clip 0.2, vf 0.5, ent 0, max grad
// norm 0.5, Adam lr 3e-4 / 0.9 / 0.999 / 1e-5, 2 epochs of minibatches of min(1 024, T E) rows, env seed 13, noise seed 13.
//
//   c_abi_ppo_example [envs = 1024] [traffic = 1] [steps = 64] [iterations = 3] [dump]
// prints
//   collect <sum obs> <sum reward> <sum values> <sum adv> <sum ret>   64-bit sums of the float32 bit patterns after the
//                                                                      first collection + GAE (obs: all T + 1 rows)
//   update <13 sums of the parameter tensors, as doubles> <value loss>   after the first minibatch update
//   final <value loss> <1 if every parameter is finite>                after the last iteration
// and, with a fifth argument, writes the 13 parameter tensors after that first update to the file `dump` as raw float32.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "acas2d.h"

#define HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define ACAS(x) do { int rc_ = (x); if (rc_ != ACAS2D_OK) { fprintf(stderr, "%s: %d %s\n", #x, rc_, acas2d_last_error()); return 3; } } while (0)

// gym_ACAS2D/settings.py:1-54 with the normalisers of game.py:120-128 / rewards.py:22-23,46-47 (as c_abi_example.cpp)
static Acas2dConfig default_config() {
    const double W = 1600, H = 1000, FPS = 100, SIZE = 24, AIRSPEED = 200, MAX_STEPS = 1000;
    const double CR = 2 * SIZE, GR = 6 * SIZE, step_len = AIRSPEED / FPS * MAX_STEPS;
    Acas2dConfig c = {};
    c.dt = 1 / FPS; c.acc_lat_limit = 20 * 9.80665; c.max_steps = (int32_t)MAX_STEPS;
    c.collision_dist = 2 * CR; c.goal_radius = GR; c.safe_distance = 4 * CR;
    c.own_x0 = CR; c.own_y0 = H / 2; c.own_v = AIRSPEED; c.own_heading0 = 0; c.own_heading_jitter = 3;
    c.goal_x = W - GR; c.goal_y = H / 2;
    const double d0 = c.goal_x - c.own_x0, diag = __builtin_sqrt(W * W + H * H);
    c.d_goal_max = d0 + step_len; c.d_dev_max = step_len; c.d_sep_max = diag + 2 * step_len;
    c.d_cpa_max = diag; c.v_closing_max = 2 * AIRSPEED;
    c.rw_d_goal_max = (W - GR - 2 * SIZE) + step_len; c.rw_d_dev_max = (W - GR - 2 * SIZE) / 2;
    c.reward_goal = 1000; c.reward_collision = -1000;
    c.t0_x = W - CR; c.t0_y_base = CR; c.t0_y_span = H - 2 * CR;
    c.t0_heading_base = 145; c.t0_heading_step = 70; c.t0_heading_jitter = 15;
    c.tn_x_max = W - SIZE; c.tn_y_max = 3 * H / 5;
    c.speed_factor_min = 1; c.speed_factor_max = 1; c.airspeed = AIRSPEED;
    return c;
}

static uint64_t g_lcg = 13;
static uint64_t lcg() { g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull; return g_lcg; }

static hipError_t dmalloc(size_t bytes, void** p) {
    hipError_t e = hipMalloc(p, bytes);
    return e == hipSuccess ? hipMemset(*p, 0, bytes) : e;
}

int main(int argc, char** argv) {
    const int64_t E = argc > 1 ? atoll(argv[1]) : 1024;
    const int32_t N = argc > 2 ? atoi(argv[2]) : 1;
    const int T = argc > 3 ? atoi(argv[3]) : 64;
    const int iterations = argc > 4 ? atoi(argv[4]) : 3;
    const char* dump = argc > 5 ? argv[5] : nullptr;
    const int D = 5 + 3 * N;
    if ((size_t)acas2d_config_size() != sizeof(Acas2dConfig) || acas2d_gae_size() != sizeof(Acas2dGae) ||
        acas2d_abi_version() != ACAS2D_ABI_VERSION) { fprintf(stderr, "header / library mismatch\n"); return 1; }
    if (E < 1 || T < 1 || iterations < 1 || (int64_t)T * E < 2) { fprintf(stderr, "bad sizes\n"); return 1; }
    const Acas2dConfig cfg = default_config();
    const uint64_t seed = 13, noise_seed = 13;
    const int64_t n = (int64_t)T * E;
    const int B = (int)(n < 1024 ? n : 1024), epochs = 2;

    // ---- the env (one zeroed allocation per array; the library allocates nothing and keeps no state)
    Acas2dState st = {};
    void** f_e[] = {&st.own_x, &st.own_y, &st.own_psi, &st.own_v, &st.goal_x, &st.goal_y, &st.total_reward, (void**)&st.steps,
                    (void**)&st.episode};
    for (void** p : f_e) HIP(dmalloc(E * 4, p));
    void** f_en[] = {&st.trf_x, &st.trf_y, &st.trf_psi, &st.trf_v};
    for (void** p : f_en) HIP(dmalloc(E * N * 4, p));
    HIP(dmalloc(E, (void**)&st.status));

    // ---- the rollout buffers: obs [T + 1][E][D] (row T: the observation the next iteration starts from), the rest [T][E]
    float *obs, *act, *reward, *values, *logp, *adv, *ret, *last_value;
    uint8_t *done, *outcome;
    HIP(dmalloc((size_t)(n + E) * D * 4, (void**)&obs));
    float** f_te[] = {&act, &reward, &values, &logp, &adv, &ret};
    for (float** p : f_te) HIP(dmalloc(n * 4, (void**)p));
    HIP(dmalloc(E * 4, (void**)&last_value));
    HIP(dmalloc(n, (void**)&done)); HIP(dmalloc(n, (void**)&outcome));

    // ---- the 13 parameter tensors, torch layouts, in the update's order
    const int count[13] = {64 * D, 64, 64 * 64, 64, 64, 1, 64 * D, 64, 64 * 64, 64, 64, 1, 1};
    const float scale[13] = {0.5f, 0, 0.25f, 0, 0.015625f, 0, 0.5f, 0, 0.25f, 0, 0.125f, 0, 0};
    std::vector<float> host[13];
    float* prm[13];
    for (int k = 0; k < 13; ++k) {
        host[k].assign(count[k], 0.0f);
        if (scale[k] != 0)
            for (float& w : host[k]) w = ((float)(lcg() >> 40) / 16777216.0f - 0.5f) * scale[k];
        HIP(dmalloc(count[k] * 4, (void**)&prm[k]));
        HIP(hipMemcpy(prm[k], host[k].data(), count[k] * 4, hipMemcpyHostToDevice));
    }
    // the transposed copies the collector and the GAE kernel read: w1t [D][64], w2t [64][64] of both nets
    float* tr[4];
    const int tr_of[4] = {0, 2, 6, 8}, tr_in[4] = {D, 64, D, 64};
    for (int q = 0; q < 4; ++q) HIP(dmalloc(count[tr_of[q]] * 4, (void**)&tr[q]));
    std::vector<float> tmp;
    auto transpose_all = [&]() -> hipError_t {
        for (int q = 0; q < 4; ++q) {
            const int k = tr_of[q], in = tr_in[q];
            hipError_t e = hipMemcpy(host[k].data(), prm[k], count[k] * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return e;
            tmp.resize(count[k]);
            for (int o = 0; o < 64; ++o) for (int i = 0; i < in; ++i) tmp[(size_t)i * 64 + o] = host[k][(size_t)o * in + i];
            e = hipMemcpy(tr[q], tmp.data(), count[k] * 4, hipMemcpyHostToDevice);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };

    // ---- the update's workspace and the GAE constants
    const int ws = acas2d_ppo_workspace_floats(D);
    if (ws <= 0) { fprintf(stderr, "obs_dim %d has no fused update (n_traffic in {1, 2, 3, 4, 8})\n", D); return 1; }
    float *grad, *adam_m, *adam_v, *stats, *gamma_d;
    int32_t* adam_step;
    int64_t* idx;
    HIP(dmalloc(ws * 4, (void**)&grad)); HIP(dmalloc(ws * 4, (void**)&adam_m)); HIP(dmalloc(ws * 4, (void**)&adam_v));
    HIP(dmalloc(8 * 4, (void**)&stats)); HIP(dmalloc(4, (void**)&adam_step)); HIP(dmalloc((size_t)B * 8, (void**)&idx));
    HIP(dmalloc(2 * 4, (void**)&gamma_d));
    const float gamma_h[2] = {0.99f, (float)(0.99 * 0.95)};          // gamma, gamma x lambda (the product in double)
    HIP(hipMemcpy(gamma_d, gamma_h, sizeof(gamma_h), hipMemcpyHostToDevice));

    hipStream_t stream;
    HIP(hipStreamCreate(&stream));
    ACAS(acas2d_reset_f32(&cfg, &st, /*mask*/ nullptr, obs, /*do_init*/ 1, seed, /*env_offset*/ 0, E, N, stream));

    auto bits_sum = [&](const float* d, size_t count_, unsigned long long* out) -> hipError_t {
        std::vector<uint32_t> h(count_);
        hipError_t e = hipMemcpy(h.data(), d, count_ * 4, hipMemcpyDeviceToHost);
        unsigned long long s = 0;
        for (uint32_t w : h) s += w;
        *out = s;
        return e;
    };
    std::vector<int64_t> perm(n);
    float vf_loss = 0;
    for (int it = 0; it < iterations; ++it) {
        HIP(hipStreamSynchronize(stream));
        HIP(transpose_all());
        // -- collect: obs[0] holds the observation the first action is drawn on, the kernel writes obs[1 .. T]
        Acas2dStepIO io = {};
        io.actions = act; io.obs = obs + (size_t)E * D; io.reward = reward; io.done = done; io.outcome = outcome;
        Acas2dActorCritic ac = {};
        ac.actor.w1t = tr[0]; ac.actor.b1 = prm[1]; ac.actor.w2t = tr[1]; ac.actor.b2 = prm[3]; ac.actor.w3 = prm[4];
        ac.actor.b3 = prm[5]; ac.actor.hidden = 64;
        ac.v1t = tr[2]; ac.vb1 = prm[7]; ac.v2t = tr[3]; ac.vb2 = prm[9]; ac.v3 = prm[10]; ac.vb3 = prm[11];
        ac.log_std = prm[12]; ac.values = values; ac.logp = logp; ac.noise_seed = noise_seed; ac.noise_step = (uint32_t)(it * T);
        ACAS(acas2d_collect_f32(&cfg, &st, &io, &ac, obs, T, seed, 0, E, N, stream));
        // -- the bootstrap value of obs[T] and GAE, one launch
        Acas2dGae g = {};
        g.reward = reward; g.value = values; g.done = done; g.obs_last = obs + (size_t)n * D;
        g.v1t = tr[2]; g.vb1 = prm[7]; g.v2t = tr[3]; g.vb2 = prm[9]; g.v3 = prm[10]; g.vb3 = prm[11];
        g.gamma = gamma_d; g.gamma_lambda = gamma_d + 1; g.adv = adv; g.ret = ret; g.last_value_out = last_value;
        g.n_envs = E; g.n_steps = T; g.n_members = 1; g.obs_dim = D;
        ACAS(acas2d_gae_f32(&g, stream));
        HIP(hipStreamSynchronize(stream));
        if (it == 0) {
            unsigned long long s[5];
            HIP(bits_sum(obs, (size_t)(n + E) * D, &s[0])); HIP(bits_sum(reward, n, &s[1])); HIP(bits_sum(values, n, &s[2]));
            HIP(bits_sum(adv, n, &s[3])); HIP(bits_sum(ret, n, &s[4]));
            printf("collect %llu %llu %llu %llu %llu\n", s[0], s[1], s[2], s[3], s[4]);
        }
        // -- the update: `epochs` passes over host-shuffled minibatches of B rows (a tail of fewer rows is dropped)
        Acas2dPpoUpdate u = {};
        u.actor_w1 = prm[0]; u.actor_b1 = prm[1]; u.actor_w2 = prm[2]; u.actor_b2 = prm[3]; u.actor_w3 = prm[4]; u.actor_b3 = prm[5];
        u.critic_w1 = prm[6]; u.critic_b1 = prm[7]; u.critic_w2 = prm[8]; u.critic_b2 = prm[9]; u.critic_w3 = prm[10];
        u.critic_b3 = prm[11]; u.log_std = prm[12];
        u.obs = obs; u.act = act; u.old_logp = logp; u.adv = adv; u.ret = ret; u.idx = idx; u.n_rows = B; u.obs_dim = D;
        u.clip_range = 0.2f; u.vf_coef = 0.5f; u.ent_coef = 0.0f; u.max_grad_norm = 0.5f;
        u.learning_rate = 3e-4f; u.beta1 = 0.9f; u.beta2 = 0.999f; u.adam_eps = 1e-5f;
        u.grad = grad; u.adam_m = adam_m; u.adam_v = adam_v; u.adam_step = adam_step; u.stats = stats;
        for (int ep = 0; ep < epochs; ++ep) {
            for (int64_t i = 0; i < n; ++i) perm[i] = i;
            for (int64_t i = n - 1; i >= 1; --i) {
                const int64_t j = (int64_t)((lcg() >> 33) % (uint64_t)(i + 1));
                const int64_t t_ = perm[i]; perm[i] = perm[j]; perm[j] = t_;
            }
            for (int64_t i = 0; i + B <= n; i += B) {
                HIP(hipMemcpyAsync(idx, perm.data() + i, (size_t)B * 8, hipMemcpyHostToDevice, stream));
                ACAS(acas2d_ppo_update_f32(&u, stream));
                HIP(hipStreamSynchronize(stream));           // (idx is rewritten by the next minibatch)
                if (it == 0 && ep == 0 && i == 0) {
                    float sh[8];
                    HIP(hipMemcpy(sh, stats, sizeof(sh), hipMemcpyDeviceToHost));
                    FILE* f = dump ? fopen(dump, "wb") : nullptr;
                    if (dump && !f) { fprintf(stderr, "cannot write %s\n", dump); return 1; }
                    printf("update");
                    for (int k = 0; k < 13; ++k) {
                        HIP(hipMemcpy(host[k].data(), prm[k], count[k] * 4, hipMemcpyDeviceToHost));
                        double s = 0;
                        for (float w : host[k]) s += (double)w;
                        printf(" %.17g", s);
                        if (f) fwrite(host[k].data(), 4, count[k], f);
                    }
                    if (f) fclose(f);
                    printf(" %.9e\n", (double)sh[5]);
                }
            }
        }
        float sh[8];
        HIP(hipMemcpy(sh, stats, sizeof(sh), hipMemcpyDeviceToHost));
        vf_loss = sh[5];
        // the next iteration starts from the observation this one ended on
        HIP(hipMemcpyAsync(obs, obs + (size_t)n * D, (size_t)E * D * 4, hipMemcpyDeviceToDevice, stream));
    }
    HIP(hipStreamSynchronize(stream));
    int finite = 1;
    for (int k = 0; k < 13; ++k) {
        HIP(hipMemcpy(host[k].data(), prm[k], count[k] * 4, hipMemcpyDeviceToHost));
        for (float w : host[k]) finite &= isfinite(w) ? 1 : 0;
    }
    printf("final %.9e %d\n", (double)vf_loss, finite);
    return 0;
}
