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

namespace {
// n sweeps of a full-batch trainer: the user half-step, then the item half-step unless the items are frozen.  half_step(side, k)
// (k = 0 .. n - 1: the sweep) returns the rows it updated; so does this, summed
template <class HalfStep>
double sweeps(int n, bool items, HalfStep &&half_step) {
    double updated = 0.0;
    for (int k = 0; k < n; ++k) {
        updated += half_step(CU2REC_SIDE_USERS, k);
        if (items) updated += half_step(CU2REC_SIDE_ITEMS, k);
    }
    return updated;
}

// The trainers that watch an objective instead of a test set (cu2rec_train_implicit, cu2rec_train_lmf): the schedule of train()
// with sweeps for the iterations and the objective for the loss.  There is no test set and the learning rate does not decay: the
// schedule's own lines and its patience stay off; the objective's line (`label`) is printed here.
// half_step(hyper, side, stream, iteration) returns the rows it updated, objective(hyper, iteration) the value at the current model
// (iteration: the sweep's number in cfg's count, the last one done for the objective).
template <class HalfStep, class Objective>
void train_by_objective(const char *label, cu2rec_config &cfg, bool verbose, double *objectives, cu2rec_train_stats *stats,
                        HalfStep &&half_step, Objective &&objective) {
    if (objectives)
        for (int i = 0; i < cfg.total_iterations; ++i) objectives[i] = std::numeric_limits<double>::quiet_NaN();
    cu2rec_hyper hyper{};
    double updated = 0.0;
    int done = 0;
    uint64_t last = 0;
    cu2rec_train_stats st{};
    train_schedule(
        cfg, false, false, 0.0, nullptr, &st, nullptr,
        [&](const cu2rec_hyper &h, uint64_t first, int n, hipStream_t s) {
            hyper = h;
            updated += sweeps(n, cfg.is_train, [&](int side, int k) { return half_step(h, side, s, first + static_cast<uint64_t>(k)); });
            done += n;
            last = first + static_cast<uint64_t>(n) - 1;
        },
        [&](bool on_train, float *mae, float *rmse) {
            *mae = *rmse = 0.f;  // no residual metrics in these models
            if (!on_train) return;
            const double L = objective(hyper, last);
            if (verbose) std::printf("TRAIN: Iteration %d GPU %s objective: %f\n", done, label, L);
            if (objectives) objectives[done - 1] = L;
        },
        [] {}, /*decay_lr=*/false);
    if (verbose) std::printf("Time taken for %d of iterations is %lf\n", cfg.total_iterations, st.seconds_total);
    st.updates = updated;
    if (stats) *stats = st;
}
}  // namespace

void train(const DeviceCsr &train_csr, const DeviceCsr &test_csr, cu2rec_config &cfg, DeviceModel &model, int mode,
           bool verbose, float *losses, cu2rec_train_stats *stats, int cg_steps = 0) {
    const bool cg = cg_steps > 0;  // reached through cu2rec_train_als_cg: the same checks under that name
    const Need need{cg ? "cu2rec_train_als_cg" : "cu2rec_train"};
    need(cfg.n_factors == model.n_factors, CU2REC_EINVAL, ": cfg.n_factors differs from the model's");
    need(train_csr.rows <= model.rows && train_csr.max_item < model.cols, CU2REC_EINVAL, ": train ratings exceed the model");
    need(test_csr.rows <= model.rows && test_csr.max_item < model.cols, CU2REC_EINVAL,
         ": test ratings name users/items the model does not have");
    hipStream_t stream = nullptr;  // the reference runs everything on the default stream
    if (mode == CU2REC_ALS) {
        // one "iteration" is one sweep.  The same loss cadence and lines; no learning rate, so no patience / decay;
        // stats->updates = rows solved
        need(cfg.n_factors <= kAlsMaxFactors, CU2REC_EUNSUPPORTED, cg ? ": n_factors up to 252 are supported" : ": CU2REC_ALS supports n_factors up to 252");
        double solved = 0.0;
        train_schedule(
            cfg, verbose, true, 0.0, losses, stats, stream,
            [&](const cu2rec_hyper &h, uint64_t, int n, hipStream_t s) {
                solved += sweeps(n, cfg.is_train, [&](int side, int) {
                    const int unsolved = model.als(train_csr, h, side, s, cg_steps);
                    return als_side(train_csr, side == CU2REC_SIDE_USERS, s).rows_with_ratings - unsolved;
                });
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

// Implicit-feedback training (include/cu2rec_amd.h: cu2rec_train_implicit): implicit sweeps and the implicit objective.
// cg_steps > 0 (cu2rec_train_implicit_cg): the same loop with conjugate-gradient half-steps.
void train_implicit(const DeviceCsr &train_csr, cu2rec_config &cfg, DeviceModel &model, float alpha, int cg_steps, bool verbose,
                    double *objectives, cu2rec_train_stats *stats) {
    require(cfg.n_factors == model.n_factors, "cu2rec_train_implicit: cfg.n_factors differs from the model's");
    require(cfg.total_iterations >= 0 && cfg.check_error > 0, "cu2rec_train_implicit: bad iteration counts");
    train_by_objective(
        "implicit", cfg, verbose, objectives, stats,
        [&](const cu2rec_hyper &h, int side, hipStream_t s, uint64_t) {
            const int unsolved = model.ials(train_csr, h, alpha, side, s, cg_steps);
            return als_side(train_csr, side == CU2REC_SIDE_USERS, s).rows_with_ratings - unsolved;
        },
        [&](const cu2rec_hyper &h, uint64_t) { return model.implicit_objective(train_csr, h, alpha, nullptr); });
}

// Logistic matrix factorization (include/cu2rec_amd.h: cu2rec_train_lmf): full-batch logistic sweeps and the log-posterior.  The
// learning rate is AdaGrad's and does not decay.
void train_lmf(const DeviceCsr &train_csr, cu2rec_config &cfg, DeviceModel &model, float alpha, bool verbose, double *objectives,
               cu2rec_train_stats *stats) {
    require(cfg.n_factors == model.n_factors, "cu2rec_train_lmf: cfg.n_factors differs from the model's");
    require(cfg.total_iterations >= 0 && cfg.check_error > 0, "cu2rec_train_lmf: bad iteration counts");
    const cu2rec_hyper hyper{cfg.learning_rate, cfg.P_reg, cfg.Q_reg, cfg.user_bias_reg, cfg.item_bias_reg};
    model.logistic_check("cu2rec_train_lmf", train_csr, hyper, alpha, {}, {});
    model.lmf_reset();
    train_by_objective(
        "logistic", cfg, verbose, objectives, stats,
        [&](const cu2rec_hyper &h, int side, hipStream_t s, uint64_t) {
            return (side == CU2REC_SIDE_USERS ? train_csr.rows : train_csr.cols) - model.lmf(train_csr, h, alpha, side, s);
        },
        [&](const cu2rec_hyper &h, uint64_t) { return model.lmf_objective(train_csr, h, alpha, nullptr); });
}

// Bayesian Personalized Ranking (include/cu2rec_amd.h: cu2rec_train_bpr): sweep t is iteration t of cfg's count, its negatives drawn
// with cfg.seed; the objective at a check is over the triples of the sweep just done.  The accumulators are the logistic trainer's.
void train_bpr(const DeviceCsr &train_csr, cu2rec_config &cfg, DeviceModel &model, bool verbose, double *objectives,
               cu2rec_train_stats *stats) {
    require(cfg.n_factors == model.n_factors, "cu2rec_train_bpr: cfg.n_factors differs from the model's");
    require(cfg.total_iterations >= 0 && cfg.check_error > 0, "cu2rec_train_bpr: bad iteration counts");
    const cu2rec_hyper hyper{cfg.learning_rate, cfg.P_reg, cfg.Q_reg, cfg.user_bias_reg, cfg.item_bias_reg};
    require(cfg.cur_iterations >= 0, "cu2rec_train_bpr: bad iteration counts");
    model.logistic_check("cu2rec_train_bpr", train_csr, hyper, {}, {},
                         static_cast<long long>(cfg.cur_iterations) + std::max(cfg.total_iterations, 1) - 1);  // the last sweep's number
    model.lmf_reset();
    const uint64_t seed = static_cast<uint64_t>(static_cast<uint32_t>(cfg.seed));
    train_by_objective(
        "BPR", cfg, verbose, objectives, stats,
        [&](const cu2rec_hyper &h, int side, hipStream_t s, uint64_t t) {
            return (side == CU2REC_SIDE_USERS ? train_csr.rows : train_csr.cols) - model.bpr(train_csr, h, seed, static_cast<int>(t), side, s);
        },
        [&](const cu2rec_hyper &h, uint64_t t) { return model.bpr_objective(train_csr, h, seed, static_cast<int>(t), nullptr, nullptr, nullptr); });
}

// Softmax matrix factorization (include/cu2rec_amd.h: cu2rec_train_softmax): full-batch softmax sweeps and their objective.  The
// accumulators are the logistic trainer's; the learning rate is AdaGrad's and does not decay.
void train_softmax(const DeviceCsr &train_csr, cu2rec_config &cfg, DeviceModel &model, bool verbose, double *objectives,
                   cu2rec_train_stats *stats) {
    require(cfg.n_factors == model.n_factors, "cu2rec_train_softmax: cfg.n_factors differs from the model's");
    require(cfg.total_iterations >= 0 && cfg.check_error > 0, "cu2rec_train_softmax: bad iteration counts");
    const cu2rec_hyper hyper{cfg.learning_rate, cfg.P_reg, cfg.Q_reg, cfg.user_bias_reg, cfg.item_bias_reg};
    model.softmax_check("cu2rec_train_softmax", train_csr, hyper, {});
    model.lmf_reset();
    train_by_objective(
        "softmax", cfg, verbose, objectives, stats,
        [&](const cu2rec_hyper &h, int side, hipStream_t s, uint64_t) {
            return (side == CU2REC_SIDE_USERS ? train_csr.rows : train_csr.cols) - model.softmax(train_csr, h, side, s);
        },
        [&](const cu2rec_hyper &h, uint64_t) { return model.softmax_objective(train_csr, h, nullptr); });
}

}  // namespace cu2rec

extern "C" int cu2rec_train_softmax(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, int verbose, double *objectives,
                                    cu2rec_train_stats *stats) {
    using namespace cu2rec;
    return guarded([&] {
        require(train && cfg && model, "cu2rec_train_softmax: null argument");
        cu2rec::train_softmax(unwrap(train), *cfg, unwrap(model), verbose != 0, objectives, stats);
    });
}

extern "C" int cu2rec_train_lmf(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, float alpha, int verbose,
                                double *objectives, cu2rec_train_stats *stats) {
    using namespace cu2rec;
    return guarded([&] {
        require(train && cfg && model, "cu2rec_train_lmf: null argument");
        cu2rec::train_lmf(unwrap(train), *cfg, unwrap(model), alpha, verbose != 0, objectives, stats);
    });
}

extern "C" int cu2rec_train_bpr(const cu2rec_csr *train, cu2rec_config *cfg, cu2rec_model *model, int verbose, double *objectives,
                                cu2rec_train_stats *stats) {
    using namespace cu2rec;
    return guarded([&] {
        require(train && cfg && model, "cu2rec_train_bpr: null argument");
        cu2rec::train_bpr(unwrap(train), *cfg, unwrap(model), verbose != 0, objectives, stats);
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
        require_cg_steps("cu2rec_train_implicit_cg", cg_steps);
        cu2rec::train_implicit(unwrap(train), *cfg, unwrap(model), alpha, cg_steps, verbose != 0, objectives, stats);
    });
}

extern "C" int cu2rec_train_als_cg(const cu2rec_csr *train, const cu2rec_csr *test, cu2rec_config *cfg, cu2rec_model *model, int cg_steps,
                                   int verbose, float *losses, cu2rec_train_stats *stats) {
    using namespace cu2rec;
    return guarded([&] {
        require(train && test && cfg && model, "cu2rec_train_als_cg: null argument");
        require_cg_steps("cu2rec_train_als_cg", cg_steps);
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
