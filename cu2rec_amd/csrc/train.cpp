// train(): the reference's training loop (training.cu:21-217) re-expressed for this library.
// Same observable schedule -- loss cadence, stdout lines, patience / learning-rate decay, what
// the clock covers (train_schedule.hpp) -- with the SGD launches between two loss checks queued back to back on one
// stream and timed by HIP events.  No ping-pong buffers, no per-iteration memset, no RNG state:
// item rows are updated in place (mf_sequential.cu semantics, the parity target) -- except in
// CU2REC_SGD_PINGPONG, which keeps the reference GPU loop's two item buffers and its loss-before-swap order.
// CU2REC_ALS runs the same schedule with exact half-steps (als.hip) in place of the SGD iterations; cg_steps > 0
// (cu2rec_train_als_cg): with conjugate-gradient half-steps (als_cg.hip).
#include "train_schedule.hpp"

namespace cu2rec {

void train(const DeviceCsr &train_csr, const DeviceCsr &test_csr, cu2rec_config &cfg, DeviceModel &model, int mode,
           bool verbose, float *losses, cu2rec_train_stats *stats, int cg_steps = 0) {
    const bool cg = cg_steps > 0;  // reached through cu2rec_train_als_cg: the same checks under that name
    require(cfg.n_factors == model.n_factors, cg ? "cu2rec_train_als_cg: cfg.n_factors differs from the model's"
                                                 : "cu2rec_train: cfg.n_factors differs from the model's");
    require(train_csr.rows <= model.rows && train_csr.max_item < model.cols,
            cg ? "cu2rec_train_als_cg: train ratings exceed the model" : "cu2rec_train: train ratings exceed the model");
    require(test_csr.rows <= model.rows && test_csr.max_item < model.cols,
            cg ? "cu2rec_train_als_cg: test ratings name users/items the model does not have"
               : "cu2rec_train: test ratings name users/items the model does not have");
    hipStream_t stream = nullptr;  // the reference runs everything on the default stream
    if (mode == CU2REC_ALS) {
        // one "iteration" is one sweep: the user half-step, then the item half-step unless the items are frozen.  The same loss
        // cadence and lines; no learning rate, so no patience / decay; stats->updates = rows solved
        if (cfg.n_factors > kAlsMaxFactors)
            fail(CU2REC_EUNSUPPORTED, cg ? "cu2rec_train_als_cg: n_factors up to 252 are supported" : "cu2rec_train: CU2REC_ALS supports n_factors up to 252");
        double solved = 0.0;
        train_schedule(
            cfg, verbose, true, 0.0, losses, stats, stream,
            [&](const cu2rec_hyper &h, uint64_t, int n, hipStream_t s) {
                for (int k = 0; k < n; ++k) {
                    const int u = model.als(train_csr, h, CU2REC_SIDE_USERS, s, cg_steps);
                    solved += train_csr.als->users.rows_with_ratings - u;
                    if (cfg.is_train) {
                        const int i = model.als(train_csr, h, CU2REC_SIDE_ITEMS, s, cg_steps);
                        solved += train_csr.als->items.rows_with_ratings - i;
                    }
                }
            },
            [&](bool on_train, float *mae, float *rmse) {
                model.loss(on_train ? train_csr : test_csr, nullptr, nullptr, mae, rmse, stream);
            },
            [] {}, /*decay_lr=*/false);
        if (stats) stats->updates = solved;
        return;
    }
    const uint64_t seed = static_cast<uint64_t>(static_cast<uint32_t>(cfg.seed));
    train_schedule(
        cfg, verbose, true, static_cast<double>(train_csr.users_with_ratings), losses, stats, stream,
        [&](const cu2rec_hyper &h, uint64_t first, int n, hipStream_t s) {
            // CU2REC_SGD_PINGPONG: the reference evaluates the loss BEFORE it swaps the item buffers (training.cu:121 vs
            // :164), i.e. on this iteration's P and the item side the iteration READ; so the last swap waits for the loss
            model.sgd(train_csr, h, seed, first, n, mode, cfg.is_train, s, /*defer_last_swap=*/mode == CU2REC_SGD_PINGPONG);
        },
        [&](bool on_train, float *mae, float *rmse) {
            model.loss(on_train ? train_csr : test_csr, nullptr, nullptr, mae, rmse, stream);
        },
        [&] { model.finish_swap(); });
}

// Implicit-feedback training (include/cu2rec_amd.h: cu2rec_train_implicit): the schedule above with implicit sweeps for the
// iterations and the objective for the loss.  There is no test set and no learning rate: the schedule's own lines and its
// patience stay off; the objective's line is printed here.  cg_steps > 0 (cu2rec_train_implicit_cg): the same loop with
// conjugate-gradient half-steps.
void train_implicit(const DeviceCsr &train_csr, cu2rec_config &cfg, DeviceModel &model, float alpha, int cg_steps, bool verbose,
                    double *objectives, cu2rec_train_stats *stats) {
    require(cfg.n_factors == model.n_factors, "cu2rec_train_implicit: cfg.n_factors differs from the model's");
    require(cfg.total_iterations >= 0 && cfg.check_error > 0, "cu2rec_train_implicit: bad iteration counts");
    hipStream_t stream = nullptr;
    if (objectives)
        for (int i = 0; i < cfg.total_iterations; ++i) objectives[i] = std::numeric_limits<double>::quiet_NaN();
    cu2rec_hyper hyper{};
    double solved = 0.0;
    int done = 0;
    cu2rec_train_stats st{};
    train_schedule(
        cfg, false, false, 0.0, nullptr, &st, stream,
        [&](const cu2rec_hyper &h, uint64_t, int n, hipStream_t s) {
            hyper = h;
            for (int k = 0; k < n; ++k) {
                const int u = model.ials(train_csr, h, alpha, CU2REC_SIDE_USERS, s, cg_steps);
                solved += train_csr.als->users.rows_with_ratings - u;
                if (cfg.is_train) {
                    const int i = model.ials(train_csr, h, alpha, CU2REC_SIDE_ITEMS, s, cg_steps);
                    solved += train_csr.als->items.rows_with_ratings - i;
                }
            }
            done += n;
        },
        [&](bool on_train, float *mae, float *rmse) {
            *mae = *rmse = 0.f;  // no residual metrics in this model
            if (!on_train) return;
            const double L = model.implicit_objective(train_csr, hyper, alpha, stream);
            if (verbose) std::printf("TRAIN: Iteration %d GPU implicit objective: %f\n", done, L);
            if (objectives) objectives[done - 1] = L;
        },
        [] {}, /*decay_lr=*/false);
    if (verbose) std::printf("Time taken for %d of iterations is %lf\n", cfg.total_iterations, st.seconds_total);
    st.updates = solved;
    if (stats) *stats = st;
}

// Logistic matrix factorization (include/cu2rec_amd.h: cu2rec_train_lmf): train_implicit's loop with full-batch logistic half-steps
// for the iterations and the log-posterior for the loss.  The learning rate is AdaGrad's and does not decay.
void train_lmf(const DeviceCsr &train_csr, cu2rec_config &cfg, DeviceModel &model, float alpha, bool verbose, double *objectives,
               cu2rec_train_stats *stats) {
    require(cfg.n_factors == model.n_factors, "cu2rec_train_lmf: cfg.n_factors differs from the model's");
    require(cfg.total_iterations >= 0 && cfg.check_error > 0, "cu2rec_train_lmf: bad iteration counts");
    cu2rec_hyper hyper{cfg.learning_rate, cfg.P_reg, cfg.Q_reg, cfg.user_bias_reg, cfg.item_bias_reg};
    model.lmf_check("cu2rec_train_lmf", train_csr, hyper, alpha, nullptr);
    model.lmf_reset();
    hipStream_t stream = nullptr;
    if (objectives)
        for (int i = 0; i < cfg.total_iterations; ++i) objectives[i] = std::numeric_limits<double>::quiet_NaN();
    double stepped = 0.0;
    int done = 0;
    cu2rec_train_stats st{};
    train_schedule(
        cfg, false, false, 0.0, nullptr, &st, stream,
        [&](const cu2rec_hyper &h, uint64_t, int n, hipStream_t s) {
            hyper = h;
            for (int k = 0; k < n; ++k) {
                stepped += train_csr.rows - model.lmf(train_csr, h, alpha, CU2REC_SIDE_USERS, s);
                if (cfg.is_train) stepped += train_csr.cols - model.lmf(train_csr, h, alpha, CU2REC_SIDE_ITEMS, s);
            }
            done += n;
        },
        [&](bool on_train, float *mae, float *rmse) {
            *mae = *rmse = 0.f;  // no residual metrics in this model
            if (!on_train) return;
            const double L = model.lmf_objective(train_csr, hyper, alpha, stream);
            if (verbose) std::printf("TRAIN: Iteration %d GPU logistic objective: %f\n", done, L);
            if (objectives) objectives[done - 1] = L;
        },
        [] {}, /*decay_lr=*/false);
    if (verbose) std::printf("Time taken for %d of iterations is %lf\n", cfg.total_iterations, st.seconds_total);
    st.updates = stepped;
    if (stats) *stats = st;
}

}  // namespace cu2rec

extern "C" int cu2rec_train_lmf(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, float alpha, int verbose,
                                double *objectives, cu2rec_train_stats *stats) {
    using namespace cu2rec;
    return guarded([&] {
        require(train && cfg && model, "cu2rec_train_lmf: null argument");
        cu2rec::train_lmf(unwrap(train), *cfg, unwrap(model), alpha, verbose != 0, objectives, stats);
    });
}

extern "C" int cu2rec_train_implicit(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, float alpha, int verbose,
                                     double *objectives, cu2rec_train_stats *stats) {
    using namespace cu2rec;
    return guarded([&] {
        require(train && cfg && model, "cu2rec_train_implicit: null argument");
        cu2rec::train_implicit(unwrap(train), *cfg, unwrap(model), alpha, 0, verbose != 0, objectives, stats);
    });
}

extern "C" int cu2rec_train_implicit_cg(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, float alpha, int cg_steps,
                                        int verbose, double *objectives, cu2rec_train_stats *stats) {
    using namespace cu2rec;
    return guarded([&] {
        require(train && cfg && model, "cu2rec_train_implicit_cg: null argument");
        require(cg_steps >= 1 && cg_steps <= CU2REC_ALS_CG_MAX_STEPS, "cu2rec_train_implicit_cg: cg_steps must be in [1, CU2REC_ALS_CG_MAX_STEPS]");
        cu2rec::train_implicit(unwrap(train), *cfg, unwrap(model), alpha, cg_steps, verbose != 0, objectives, stats);
    });
}

extern "C" int cu2rec_train_als_cg(const cu2rec_csr *train, const cu2rec_csr *test, cu2rec_config *cfg, cu2rec_model *model, int cg_steps,
                                   int verbose, float *losses, cu2rec_train_stats *stats) {
    using namespace cu2rec;
    return guarded([&] {
        require(train && test && cfg && model, "cu2rec_train_als_cg: null argument");
        require(cg_steps >= 1 && cg_steps <= CU2REC_ALS_CG_MAX_STEPS, "cu2rec_train_als_cg: cg_steps must be in [1, CU2REC_ALS_CG_MAX_STEPS]");
        cu2rec::train(unwrap(train), unwrap(test), *cfg, unwrap(model), CU2REC_ALS, verbose != 0, losses, stats, cg_steps);
    });
}

extern "C" int cu2rec_train(const cu2rec_csr *train, const cu2rec_csr *test, cu2rec_config *cfg, cu2rec_model *model,
                            int mode, int verbose, float *losses, cu2rec_train_stats *stats) {
    using namespace cu2rec;
    return guarded([&] {
        require(train && test && cfg && model, "cu2rec_train: null argument");
        cu2rec::train(unwrap(train), unwrap(test), *cfg, unwrap(model), mode, verbose != 0, losses, stats);
    });
}
