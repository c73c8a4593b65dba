// bin/mf -- trains a matrix-factorisation model on the GPU and writes its five components.
// Drop-in for the reference CLI (mf.cu:16-99): same arguments, same stdout lines, same output
// files; built on the C ABI of libcu2rec_amd.
//
//   bin/mf [-c config] [-m blocksolve|ordered|hogwild|serial|pingpong|als|alscg|svd|softmax|ials|lmf|bpr|knn|ease|slim] [-a alpha] [-C cg_steps] [-g gpus]
//          [-s sync_every] [-w adaptive|mean|weighted|sum] [-W count|cosine|tfidf|bm25] [-N neighbours] [-L l2] [-l l1] [-n sweeps] [-k K [-t T]] train.csv test.csv
// Default mode: blocksolve -- mf_sequential.cu's result within float rounding (the mode bench.py certifies against the
// 1e-4 RMSE bar); n_factors above 252, where block-solve is not compiled, falls back to `ordered` (the same result bit
// for bit).  `-m hogwild` opts into sgd.cu's own racy semantics (fastest, 1e-3 away from the sequential result while
// the model is still moving).  `-m als` trains by alternating least squares instead of SGD: total_iterations sweeps (user
// half-step, item half-step) with the config's regularisers, no learning rate; single GPU, n_factors up to 252.
// `-m alscg` is `-m als` by conjugate gradients: rows of at most 1,024 ratings take -C steps (default 3) per half-step instead of
// the exact solve (cu2rec_train_als_cg).
// `-m ials` is its implicit-feedback form (-a alpha: the confidence weight per unit of r); with -C steps its rows of at most 1,024
// entries take that many conjugate-gradient steps per sweep instead of the exact solve (cu2rec_train_implicit_cg).
// `-m lmf` trains by logistic matrix factorization (cu2rec_train_lmf): total_iterations full-batch sweeps with AdaGrad at the config's
// learning rate, -a alpha the weight per unit of r (default 1 here, not ials's 40); single GPU, no -C.  The AdaGrad accumulators
// are not written out: a run started from the five files begins them at zero.
// `-m bpr` trains by Bayesian Personalized Ranking (cu2rec_train_bpr): total_iterations deterministic full-batch sweeps over one
// sampled negative per stored entry (the config's seed), AdaGrad at the config's learning rate; single GPU, no -a, no -C.  Like
// `-m ials` and `-m lmf` it reads the test file only for -k.
// `-m softmax` trains by softmax matrix factorization (cu2rec_train_softmax): total_iterations full-batch sweeps under the multinomial
// likelihood, AdaGrad at the config's learning rate, the stored values as weights; user biases stay as they start.  It reads the test
// file only for -k, writes the five files, and refuses -a, -C, -g, -s, -w, -W, -N, -L, -l and -n.
// `-m knn` trains nothing: it builds the item-neighbourhood recommender (cu2rec_knn_create) on the training file -- -W the weighting
// (default cosine; bm25 with k1 = 100, b = 0.8), -N the neighbours kept per item (default 20, at most 256) -- writes every item's list to
// <base>_knn_ids.csv and <base>_knn_sims.csv (items x N, -1 / nan padding) where the five files would go, and prints -k's ranking line
// with the training rows as history and exclusion (cu2rec_knn_rank_metrics).  -k is required; no config is read, so -c is refused, as
// are -a, -C, -g, -s and -w.
// `-m ease` trains nothing either: it builds the closed-form item x item weights B (cu2rec_ease_create) on the training file -- -L the
// regulariser l2 (default 500) -- writes B to <base>_ease_b.csv (items x items) when there are at most 4,096 items (more: the file is
// skipped, with a word on stderr), and prints -k's ranking line with the training rows as history and exclusion
// (cu2rec_ease_rank_metrics).  -k is required; -c, -a, -C, -g, -s, -w, -W and -N are refused.
// `-m slim` is `-m ease` with SLIM's sparse weights W in B's place (cu2rec_slim_create: non-negative weights, tol 1e-3): -l the L1
// penalty l1 (default 5), -L l2 (default 500), -n the most sweeps of coordinate descent (default 10).  It writes W to <base>_slim_w.csv
// under the same 4,096-item rule, prints one line with the sweeps run, the last sweep's largest change and the nonzeros of W, then
// -k's ranking line.  It refuses what -m ease refuses; -l and -n are refused without it.
// `-m svd` builds PureSVD (cu2rec_train_svd): the config's total_iterations sweeps of block subspace iteration at its n_factors, from the
// seed-42 item factors (another seed in the config draws them again) -- no learning rate, no regulariser.  It writes the five files, both
// bias files zero and the global bias 0 (the scores are p . q), prints one line with the sweeps and the captured and total squared
// norms, and with -k the ranking line.  Single GPU; it refuses -a, -C, -g, -s, -w, -W, -N, -L, -l and -n.
// -g N (N > 1): one process per GPU -- the program forks N - 1 more ranks before anything touches a GPU, rank r takes
// device r and a contiguous range of users, the ranks train through cu2rec_train_sharded (RCCL all-reduce of the item
// deltas every -s iterations, default one epoch), rank 0 prints the lines and writes the five files.
// -k K (single GPU): after the five files, one more line -- the trained model's ranking quality at K on the test file, the
// training ratings excluded (cu2rec_model_rank_metrics); -t T: a test rating is relevant when >= T (default: every rating).
#include <getopt.h>
#include <hip/hip_runtime_api.h>
#include <signal.h>
#include <sys/prctl.h>
#include <sys/wait.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "cu2rec.hpp"

namespace {

bool g_mode_given = false;  // -m on the command line

// what -m names: one of the SGD modes (a cu2rec_sgd_mode, through cu2rec_train), or a full-batch trainer with an entry point of its own
enum class Trainer { Sgd, Als, AlsCg, Ials, Lmf, Bpr, Softmax, Knn, Ease, Slim, Svd };

// the default mode is block-solve; where it is not compiled (n_factors > 252) the default becomes `ordered`: the same
// sequential result, bit for bit instead of within float rounding
int effective_mode(int mode, int n_factors) {
    return (!g_mode_given && mode == CU2REC_SGD_BLOCKSOLVE && n_factors > 252) ? CU2REC_SGD_ORDERED : mode;
}

// all of fd or an exception
void write_all(int fd, const void *buf, size_t n) {
    const char *p = static_cast<const char *>(buf);
    while (n) {
        const ssize_t k = ::write(fd, p, n);
        if (k <= 0) throw std::runtime_error("pipe write failed");
        p += k;
        n -= static_cast<size_t>(k);
    }
}

void read_all(int fd, void *buf, size_t n) {
    char *p = static_cast<char *>(buf);
    while (n) {
        const ssize_t k = ::read(fd, p, n);
        if (k <= 0) throw std::runtime_error("pipe read failed (a rank died?)");
        p += k;
        n -= static_cast<size_t>(k);
    }
}

// One rank of `bin/mf -g N`.  to_child / from_child: rank 0's pipes to and from every other rank; up / down: this
// rank's pipes to and from rank 0.
int run_rank(int rank, int nranks, int mode, int sync_every, int merge, const std::string &config_path,
             const std::string &train_path, const std::string &test_path, const std::vector<int> &to_child,
             const std::vector<int> &from_child, int up, int down) {
#ifdef CU2REC_TEST_HOOKS
    // fault injection for the failure-propagation test (tests/test_host_abi.py), before anything touches a GPU -- compiled into
    // the test binary build/test/mf_hooks only (make -C cu2rec_amd/csrc test-hooks), never into bin/mf:
    // CU2REC_TEST_RANK_EXIT="r:code" makes rank r end with that exit code, CU2REC_TEST_RANK_HANG="r" makes rank r sit still
    // the way a rank inside a collective whose peer died would
    if (const char *env = std::getenv("CU2REC_TEST_RANK_EXIT")) {
        int r = -1, code = 0;
        if (std::sscanf(env, "%d:%d", &r, &code) == 2 && r == rank) _exit(code);
    }
    if (const char *env = std::getenv("CU2REC_TEST_RANK_HANG"))
        if (std::atoi(env) == rank) std::this_thread::sleep_for(std::chrono::seconds(120));
#endif
    if (cu2rec_device_count() < nranks) throw std::runtime_error("fewer HIP devices than ranks (-g)");
    cu2rec::check(cu2rec_set_device(rank));
    if (rank == 0) {
        size_t free_bytes = 0, total_bytes = 0;  // mf.cu:33-37
        if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) throw std::runtime_error("hipMemGetInfo failed");
        std::printf("Free memory: %ld\n\n", static_cast<long>(free_bytes));
    }
    cu2rec::HostCsr train = cu2rec::load_ratings(train_path);  // every rank parses the files and keeps its slice
    cu2rec::HostCsr test = cu2rec::load_ratings(test_path);
    if (train.nnz == 0) throw std::runtime_error("no ratings read from " + train_path);
    if (test.rows > train.rows || test.cols > train.cols) throw std::runtime_error("the test file names users / items the training file does not have");
    cu2rec_config cfg;
    cu2rec::check(cu2rec_config_default(&cfg));
    if (!config_path.empty()) cu2rec::check(cu2rec_config_read(config_path.c_str(), &cfg));
    if (rank == 0) cu2rec::check(cu2rec_config_print(&cfg));
    mode = effective_mode(mode, cfg.n_factors);

    std::vector<int> bounds(static_cast<size_t>(nranks) + 1);
    cu2rec::check(cu2rec_shard_plan(train.rows, nranks, bounds.data()));
    const int u0 = bounds[rank], u1 = bounds[rank + 1], f = cfg.n_factors;
    test.indptr.resize(static_cast<size_t>(train.rows) + 1, test.nnz);  // a test file may name fewer users (mf.cu:50-51)
    test.rows = train.rows;
    auto slice = [&](const cu2rec::HostCsr &m) {
        cu2rec::HostCsr s;
        s.rows = u1 - u0;
        s.cols = train.cols;
        s.indptr.resize(static_cast<size_t>(s.rows) + 1);
        int off = 0;
        cu2rec::check(cu2rec_csr_slice(m.indptr.data(), m.rows, u0, u1, s.indptr.data(), &off, &s.nnz));
        s.indices.assign(m.indices.begin() + off, m.indices.begin() + off + s.nnz);
        s.data.assign(m.data.begin() + off, m.data.begin() + off + s.nnz);
        s.global_bias = train.global_bias;
        return s;
    };
    const cu2rec::HostCsr tr = slice(train), te = slice(test);
    // every rank draws the reference's seed-42 initialisation and keeps its slice (training.cu:28,54)
    std::vector<float> P0(static_cast<size_t>(train.rows) * f), ub0(train.rows);
    cu2rec::check(cu2rec_init_normal(P0.data(), P0.size(), f, 0.f, 1.f, 42));
    cu2rec::check(cu2rec_init_normal(ub0.data(), ub0.size(), f, 0.f, 1.f, 42));
    cu2rec::CsrHandle d_train(tr), d_test(te);
    cu2rec::ModelHandle model(u1 - u0, train.cols, f, train.global_bias, P0.data() + static_cast<size_t>(u0) * f, nullptr,
                              ub0.data() + u0, nullptr);

    unsigned char uid[128] = {0};
    if (rank == 0) {
        cu2rec::check(cu2rec_comm_unique_id(uid));
        for (int r = 1; r < nranks; ++r) write_all(to_child[r], uid, sizeof(uid));
    } else {
        read_all(down, uid, sizeof(uid));
    }
    cu2rec_comm *comm = nullptr;
    cu2rec::check(cu2rec_comm_create(uid, rank, nranks, &comm));
    cu2rec_shard_options opt{sync_every, merge};
    cu2rec_shard_job *job = nullptr;
    cu2rec::check(cu2rec_shard_job_create(comm, model.h, d_train.h, u0, &opt, &job));
    std::vector<float> losses(static_cast<size_t>(cfg.total_iterations > 0 ? cfg.total_iterations : 1));
    cu2rec::check(cu2rec_train_sharded(job, d_test.h, &cfg, mode, 1, losses.data(), nullptr));

    std::vector<float> P(static_cast<size_t>(u1 - u0) * f), ub(u1 - u0), Q, ib;
    if (rank == 0) {
        Q.resize(static_cast<size_t>(train.cols) * f);
        ib.resize(train.cols);
    }
    cu2rec::check(cu2rec_model_download(model.h, P.data(), rank == 0 ? Q.data() : nullptr, ub.data(), rank == 0 ? ib.data() : nullptr));
    cu2rec_shard_job_destroy(job);
    cu2rec_comm_destroy(comm);
    if (rank != 0) {  // the user side goes to rank 0 through the pipe
        write_all(up, P.data(), P.size() * sizeof(float));
        write_all(up, ub.data(), ub.size() * sizeof(float));
        return 0;
    }
    std::vector<float> P_all(static_cast<size_t>(train.rows) * f), ub_all(train.rows);
    std::copy(P.begin(), P.end(), P_all.begin());
    std::copy(ub.begin(), ub.end(), ub_all.begin());
    for (int r = 1; r < nranks; ++r) {
        read_all(from_child[r], P_all.data() + static_cast<size_t>(bounds[r]) * f, static_cast<size_t>(bounds[r + 1] - bounds[r]) * f * sizeof(float));
        read_all(from_child[r], ub_all.data() + bounds[r], static_cast<size_t>(bounds[r + 1] - bounds[r]) * sizeof(float));
    }
    std::string parent_dir = ".", filename = train_path;  // mf.cu:65-87
    const size_t slash = train_path.find_last_of('/');
    if (slash != std::string::npos) {
        parent_dir = train_path.substr(0, slash);
        filename = train_path.substr(slash + 1);
    }
    const std::string base = filename.substr(0, filename.find_last_of('.'));
    const float gb = train.global_bias;
    cu2rec::check(cu2rec_write_component(parent_dir.c_str(), base.c_str(), "p", P_all.data(), train.rows, f, f));
    cu2rec::check(cu2rec_write_component(parent_dir.c_str(), base.c_str(), "q", Q.data(), train.cols, f, f));
    cu2rec::check(cu2rec_write_component(parent_dir.c_str(), base.c_str(), "user_bias", ub_all.data(), train.rows, 1, f));
    cu2rec::check(cu2rec_write_component(parent_dir.c_str(), base.c_str(), "item_bias", ib.data(), train.cols, 1, f));
    cu2rec::check(cu2rec_write_component(parent_dir.c_str(), base.c_str(), "global_bias", &gb, 1, 1, f));
    return 0;
}

// bin/mf -g N: forks the other ranks BEFORE any HIP call (a process that has initialised the GPU must not fork into
// another GPU user), wires the pipes, runs rank 0 here and collects the children's exit codes.
// A rank that fails must not leave the others sitting in a collective: every child dies with its parent (PR_SET_PDEATHSIG),
// and while rank 0 trains a watcher thread reaps the children -- the first one that ends abnormally makes the program kill
// the rest and exit non-zero at once (fresh exits only: nothing here re-executes a process that has touched a GPU).
int run_multi_gpu(int nranks, int mode, int sync_every, int merge, const std::string &config_path, const std::string &train_path,
                  const std::string &test_path) {
    std::vector<int> to_child(nranks, -1), from_child(nranks, -1);
    std::vector<pid_t> pids(nranks, 0);
    const pid_t parent = getpid();
    for (int r = 1; r < nranks; ++r) {
        int down[2], up[2];
        if (pipe(down) != 0 || pipe(up) != 0) return 2;
        const pid_t pid = fork();
        if (pid < 0) return 2;
        if (pid == 0) {
            prctl(PR_SET_PDEATHSIG, SIGKILL);
            if (getppid() != parent) _exit(2);  // the parent was gone before the request took effect
            close(down[1]);
            close(up[0]);
            for (int q = 1; q < r; ++q) {
                close(to_child[q]);
                close(from_child[q]);
            }
            int rc = 0;
            try {
                rc = run_rank(r, nranks, mode, sync_every, merge, config_path, train_path, test_path, {}, {}, up[1], down[0]);
            } catch (const std::exception &e) {
                std::cerr << "mf (rank " << r << "): " << e.what() << "\n";
                rc = 2;
            }
            _exit(rc);
        }
        close(down[0]);
        close(up[1]);
        to_child[r] = down[1];
        from_child[r] = up[0];
        pids[r] = pid;
    }
    std::vector<std::atomic<int>> reaped(nranks);  // 0: running, 1: ended cleanly
    for (auto &v : reaped) v.store(0);
    std::atomic<bool> finished{false};
    auto kill_children = [&] {
        for (int r = 1; r < nranks; ++r)
            if (!reaped[r].load()) kill(pids[r], SIGKILL);
    };
    std::thread watcher([&] {
        while (!finished.load()) {
            for (int r = 1; r < nranks; ++r) {
                if (reaped[r].load()) continue;
                int status = 0;
                const pid_t got = waitpid(pids[r], &status, WNOHANG);
                if (got != pids[r]) continue;
                if (WIFEXITED(status) && WEXITSTATUS(status) == 0) {
                    reaped[r].store(1);
                    continue;
                }
                std::cerr << "mf: rank " << r << " ended abnormally (" << (WIFSIGNALED(status) ? "signal " : "exit code ")
                          << (WIFSIGNALED(status) ? WTERMSIG(status) : WEXITSTATUS(status)) << "); stopping the other ranks\n";
                reaped[r].store(1);
                kill_children();
                for (int q = 1; q < nranks; ++q)
                    if (!reaped[q].load()) (void)waitpid(pids[q], &status, 0);  // SIGKILL: at once
                std::fflush(stdout);  // the TRAIN: / TEST: lines rank 0 has printed so far are not lost with the process
                std::fflush(stderr);
                _exit(3);  // rank 0 (this process) may be inside a collective that will never complete
            }
            std::this_thread::sleep_for(std::chrono::milliseconds(20));
        }
    });
    int rc = 0;
    try {
        rc = run_rank(0, nranks, mode, sync_every, merge, config_path, train_path, test_path, to_child, from_child, -1, -1);
    } catch (const std::exception &e) {
        std::cerr << "mf: " << e.what() << "\n";
        rc = 2;
    }
    finished.store(true);
    watcher.join();
    if (rc != 0) kill_children();  // rank 0 failed: the others may be waiting for it in a collective
    for (int r = 1; r < nranks; ++r) {
        close(to_child[r]);
        close(from_child[r]);
        if (reaped[r].load()) continue;
        int status = 0;
        if (waitpid(pids[r], &status, 0) < 0 || !WIFEXITED(status) || WEXITSTATUS(status) != 0) rc = rc ? rc : 2;
    }
    return rc;
}

// the directory and the base name the output files of a training file go by (mf.cu:65-87)
void output_place(const std::string &train_path, std::string &parent_dir, std::string &base) {
    parent_dir = ".";
    std::string filename = train_path;
    const size_t slash = train_path.find_last_of('/');
    if (slash != std::string::npos) {
        parent_dir = train_path.substr(0, slash);
        filename = train_path.substr(slash + 1);
    }
    base = filename.substr(0, filename.find_last_of('.'));
}

void print_rank_line(const cu2rec_rank_metrics &rm, int K) {
    std::printf("TEST: Precision@%d: %f Recall@%d: %f NDCG@%d: %f MAP@%d: %f HitRate@%d: %f Users: %d Skipped: %d\n", K, rm.precision, K,
                rm.recall, K, rm.ndcg, K, rm.map, K, rm.hit_rate, rm.users_evaluated, rm.users_skipped);
}

// bin/mf -m knn: the neighbour lists of the training file to <base>_knn_ids.csv / <base>_knn_sims.csv, then -k's ranking line
int run_knn(const cu2rec::HostCsr &train, cu2rec::HostCsr test, const std::string &train_path, int weighting, int neighbours, int rank_k,
            float rank_threshold) {
    if (test.rows > train.rows || test.cols > train.cols)
        throw std::runtime_error("the test file names users / items the training file does not have");
    if (train.cols > (1 << 24)) throw std::runtime_error("-m knn writes item ids through the float writer: more than 2^24 items");
    test.cols = train.cols;  // the recommender's lists and the test rows name one catalogue
    cu2rec::CsrHandle d_train(train), d_test(test);
    cu2rec::KnnHandle knn(d_train, weighting, 100.f, 0.8f, neighbours);
    const size_t total = static_cast<size_t>(train.cols) * neighbours;
    std::vector<int> ids(total);
    std::vector<float> sims(total), ids_f(total);
    cu2rec::check(cu2rec_knn_neighbors(knn.h, nullptr, train.cols, neighbours, ids.data(), sims.data()));
    for (size_t t = 0; t < total; ++t) ids_f[t] = static_cast<float>(ids[t]);
    std::string parent_dir, base;
    output_place(train_path, parent_dir, base);
    cu2rec::check(cu2rec_write_csv((parent_dir + "/" + base + "_knn_ids.csv").c_str(), ids_f.data(), train.cols, neighbours));
    cu2rec::check(cu2rec_write_csv((parent_dir + "/" + base + "_knn_sims.csv").c_str(), sims.data(), train.cols, neighbours));
    cu2rec_rank_metrics rm;
    cu2rec::check(cu2rec_knn_rank_metrics(knn.h, d_train.h, d_train.h, d_test.h, rank_k, rank_threshold, &rm, nullptr));
    print_rank_line(rm, rank_k);
    return 0;
}

// bin/mf -m ease and -m slim: the model's weights of the training file to <base><suffix> (at most kEaseCsvItems items), then -k's
// ranking line
constexpr int kEaseCsvItems = 4096;
int serve_ease(const cu2rec::EaseHandle &ease, const cu2rec::HostCsr &train, const cu2rec::CsrHandle &d_train, const cu2rec::CsrHandle &d_test,
               const std::string &train_path, const char *suffix, int rank_k, float rank_threshold) {
    std::string parent_dir, base;
    output_place(train_path, parent_dir, base);
    if (train.cols <= kEaseCsvItems) {
        std::vector<float> b(static_cast<size_t>(train.cols) * train.cols);
        cu2rec::check(cu2rec_ease_weights(ease.h, nullptr, train.cols, b.data()));
        cu2rec::check(cu2rec_write_csv((parent_dir + "/" + base + suffix).c_str(), b.data(), train.cols, train.cols));
    } else {
        std::cerr << "mf: " << train.cols << " items: " << base << suffix << " is skipped (written for at most " << kEaseCsvItems << " items)\n";
    }
    cu2rec_rank_metrics rm;
    cu2rec::check(cu2rec_ease_rank_metrics(ease.h, d_train.h, d_train.h, d_test.h, rank_k, rank_threshold, &rm, nullptr));
    print_rank_line(rm, rank_k);
    return 0;
}

// slim: null for -m ease; else -m slim's l1 and most sweeps
struct SlimOptions {
    float l1;
    int sweeps;
};
int run_ease(const cu2rec::HostCsr &train, cu2rec::HostCsr test, const std::string &train_path, float l2, const SlimOptions *slim, int rank_k,
             float rank_threshold) {
    if (test.rows > train.rows || test.cols > train.cols)
        throw std::runtime_error("the test file names users / items the training file does not have");
    test.cols = train.cols;  // the recommender's lists and the test rows name one catalogue
    cu2rec::CsrHandle d_train(train), d_test(test);
    if (!slim) return serve_ease(cu2rec::EaseHandle(d_train, l2), train, d_train, d_test, train_path, "_ease_b.csv", rank_k, rank_threshold);
    cu2rec_slim_report report;
    cu2rec::EaseHandle model(d_train, slim->l1, l2, true, slim->sweeps, 1e-3f, &report);
    std::printf("SLIM: l1: %g l2: %g Sweeps: %d LastDelta: %g Nonzeros: %lld of %lld\n", slim->l1, l2, report.sweeps, report.last_delta,
                report.nonzeros, static_cast<long long>(train.cols) * train.cols);
    return serve_ease(model, train, d_train, d_test, train_path, "_slim_w.csv", rank_k, rank_threshold);
}

}  // namespace

int main(int argc, char **argv) {
    const char *usage = "usage: mf [-c config] [-m blocksolve|ordered|hogwild|serial|pingpong|als|alscg|svd|softmax|ials|lmf|bpr|knn|ease|slim] [-a alpha] [-C cg_steps] [-g gpus] "
                        "[-s sync_every] [-w adaptive|mean|weighted|sum] [-W count|cosine|tfidf|bm25] [-N neighbours] [-L l2] [-l l1] [-n sweeps] [-k K [-t T]] train.csv test.csv\n";
    if (argc < 2) {  // mf.cu:17-19 (the reference says nothing; the usage line goes to stderr)
        std::cerr << usage;
        return -1;
    }
    std::string config_path;
    int mode = CU2REC_SGD_BLOCKSOLVE;  // the mode that meets the north star's 1e-4 bar; -m hogwild is the opt-in
    int gpus = 1, sync_every = 0, merge = CU2REC_MERGE_ADAPTIVE;
    int rank_k = 0;  // -k: 0 = no ranking line
    bool rank_given = false;
    float rank_threshold = -INFINITY;
    Trainer trainer = Trainer::Sgd;
    const char *trainer_name = "";  // -m's word, for a refusal
    float alpha = 40.f;     // -a: the weight per unit of r of -m ials (default 40) and -m lmf (default 1)
    bool alpha_given = false;
    bool cg_given = false;  // -C steps: -m ials by conjugate gradients (cu2rec_train_implicit_cg), or -m alscg's step count (default 3)
    long cg_steps = 0;
    bool sync_given = false, merge_given = false;  // -s / -w: read by -g's ranks only; -m knn refuses them
    bool weighting_given = false, neighbours_given = false;  // -W / -N: -m knn's weighting (-1: not one of the four) and list length
    int weighting = CU2REC_KNN_COSINE;
    long neighbours = 20;
    bool l2_given = false;  // -L: the regulariser of -m ease and -m slim
    float l2 = 500.f;
    bool l1_given = false, sweeps_given = false;  // -l / -n: -m slim's L1 penalty and most sweeps
    float l1 = 5.f;
    long sweeps = 10;
    int opt;
    while ((opt = getopt(argc, argv, "c:m:g:s:w:k:t:a:C:W:N:L:l:n:")) != -1) {
        switch (opt) {
            case 'a': {
                char *end = nullptr;
                alpha_given = true;
                alpha = std::strtof(optarg, &end);
                if (end == optarg || *end != '\0') alpha = NAN;  // not a number: refused below
                break;
            }
            case 'C': {
                char *end = nullptr;
                cg_given = true;
                cg_steps = std::strtol(optarg, &end, 10);
                if (end == optarg || *end != '\0') cg_steps = 0;  // not a number: refused below
                break;
            }
            case 'W':
                weighting_given = true;
                weighting = std::strcmp(optarg, "count") == 0    ? CU2REC_KNN_COUNT
                            : std::strcmp(optarg, "cosine") == 0 ? CU2REC_KNN_COSINE
                            : std::strcmp(optarg, "tfidf") == 0  ? CU2REC_KNN_TFIDF
                            : std::strcmp(optarg, "bm25") == 0   ? CU2REC_KNN_BM25
                                                                 : -1;  // refused below
                break;
            case 'N': {
                char *end = nullptr;
                neighbours_given = true;
                neighbours = std::strtol(optarg, &end, 10);
                if (end == optarg || *end != '\0') neighbours = 0;  // not a number: refused below
                break;
            }
            case 'L': {
                char *end = nullptr;
                l2_given = true;
                l2 = std::strtof(optarg, &end);
                if (end == optarg || *end != '\0') l2 = NAN;  // not a number: refused below
                break;
            }
            case 'l': {
                char *end = nullptr;
                l1_given = true;
                l1 = std::strtof(optarg, &end);
                if (end == optarg || *end != '\0') l1 = NAN;  // not a number: refused below
                break;
            }
            case 'n': {
                char *end = nullptr;
                sweeps_given = true;
                sweeps = std::strtol(optarg, &end, 10);
                if (end == optarg || *end != '\0') sweeps = 0;  // not a number: refused below
                break;
            }
            case 'k':
                rank_given = true;
                rank_k = std::atoi(optarg);
                break;
            case 't': {
                char *end = nullptr;
                rank_threshold = std::strtof(optarg, &end);
                if (end == optarg || *end != '\0') rank_threshold = NAN;  // not a number: refused below
                break;
            }
            case 'g':
                gpus = std::atoi(optarg);
                break;
            case 's':
                sync_given = true;
                sync_every = std::atoi(optarg);
                break;
            case 'w':
                merge_given = true;
                merge = std::strcmp(optarg, "mean") == 0       ? CU2REC_MERGE_MEAN
                        : std::strcmp(optarg, "sum") == 0      ? CU2REC_MERGE_SUM
                        : std::strcmp(optarg, "adaptive") == 0 ? CU2REC_MERGE_ADAPTIVE
                                                               : CU2REC_MERGE_WEIGHTED;
                break;
            case 'c':
                config_path = optarg;
                break;
            case 'm':
                g_mode_given = true;
                trainer_name = optarg;
                trainer = std::strcmp(optarg, "als") == 0     ? Trainer::Als
                          : std::strcmp(optarg, "alscg") == 0 ? Trainer::AlsCg
                          : std::strcmp(optarg, "ials") == 0  ? Trainer::Ials
                          : std::strcmp(optarg, "lmf") == 0   ? Trainer::Lmf
                          : std::strcmp(optarg, "bpr") == 0   ? Trainer::Bpr
                          : std::strcmp(optarg, "softmax") == 0 ? Trainer::Softmax
                          : std::strcmp(optarg, "knn") == 0   ? Trainer::Knn
                          : std::strcmp(optarg, "ease") == 0  ? Trainer::Ease
                          : std::strcmp(optarg, "slim") == 0  ? Trainer::Slim
                          : std::strcmp(optarg, "svd") == 0   ? Trainer::Svd
                                                              : Trainer::Sgd;
                mode = trainer != Trainer::Sgd                  ? CU2REC_ALS
                       : std::strcmp(optarg, "serial") == 0     ? CU2REC_SGD_SERIAL
                       : std::strcmp(optarg, "ordered") == 0    ? CU2REC_SGD_ORDERED
                       : std::strcmp(optarg, "pingpong") == 0   ? CU2REC_SGD_PINGPONG
                       : std::strcmp(optarg, "blocksolve") == 0 ? CU2REC_SGD_BLOCKSOLVE
                                                                : CU2REC_SGD_HOGWILD;
                break;
            default:
                std::cout << "Unknown option.\n";  // mf.cu:27-29
                return 1;
        }
    }
    if (optind + 2 > argc) {
        std::cerr << usage;
        return -1;
    }
    if (rank_given && (rank_k < 1 || rank_k > 256)) {
        std::cerr << "mf: -k must be between 1 and 256\n";
        return 1;
    }
    if (std::isnan(rank_threshold)) {
        std::cerr << "mf: -t must be a number\n";
        return 1;
    }
    if (trainer == Trainer::Knn &&
        (!rank_given || alpha_given || cg_given || gpus > 1 || !config_path.empty() || sync_given || merge_given)) {  // before the GPU is touched
        std::cerr << "mf: -m knn needs -k, reads no config (no -c), takes no -a and no -C, and is single-GPU only (no -g, -s, -w)\n" << usage;
        return 1;
    }
    if (trainer == Trainer::Svd && (alpha_given || cg_given || gpus > 1 || sync_given || merge_given || weighting_given || neighbours_given ||
                                    l2_given || l1_given || sweeps_given)) {  // before the GPU is touched
        std::cerr << "mf: -m svd takes no -a, -C, -W, -N, -L, -l or -n (its sweeps are the config's total_iterations), and is single-GPU only (no -g, -s, -w)\n"
                  << usage;
        return 1;
    }
    const bool is_slim = trainer == Trainer::Slim;
    if ((trainer == Trainer::Ease || is_slim) && (!rank_given || alpha_given || cg_given || gpus > 1 || !config_path.empty() || sync_given || merge_given ||
                                     weighting_given || neighbours_given)) {  // before the GPU is touched
        std::cerr << "mf: -m " << trainer_name << " needs -k, reads no config (no -c), takes no -a, no -C, no -W and no -N, and is single-GPU only (no -g, -s, -w)\n"
                  << usage;
        return 1;
    }
    if (l2_given && ((trainer != Trainer::Ease && !is_slim) || !(std::isfinite(l2) && l2 > 0.f))) {
        std::cerr << "mf: -L needs -m ease or -m slim and a finite l2 > 0\n" << usage;
        return 1;
    }
    if ((l1_given || sweeps_given) && (!is_slim || !(std::isfinite(l1) && l1 >= 0.f) || sweeps < 1 || sweeps > 1000000)) {
        std::cerr << "mf: -l and -n need -m slim, a finite l1 >= 0 and between 1 and 1000000 sweeps\n" << usage;
        return 1;
    }
    if (rank_given && gpus > 1) {
        std::cerr << "mf: -k is single-GPU only (not with -g)\n";
        return 1;
    }
    const bool takes_cg = trainer == Trainer::Ials || trainer == Trainer::AlsCg;
    const bool takes_alpha = trainer == Trainer::Ials || trainer == Trainer::Lmf;
    if (cg_given && (!takes_cg || cg_steps < 1 || cg_steps > CU2REC_ALS_CG_MAX_STEPS)) {  // before the GPU is touched
        std::cerr << "mf: -C needs -m ials or -m alscg and a step count between 1 and " << CU2REC_ALS_CG_MAX_STEPS << "\n" << usage;
        return 1;
    }
    if (trainer == Trainer::AlsCg && !cg_given) cg_steps = 3;
    if (trainer == Trainer::Lmf && gpus > 1) {  // before the GPU is touched
        std::cerr << "mf: -m lmf is single-GPU only (not with -g)\n" << usage;
        return 1;
    }
    if (trainer == Trainer::Bpr && (alpha_given || cg_given || gpus > 1)) {  // before the GPU is touched
        std::cerr << "mf: -m bpr takes no -a and no -C, and is single-GPU only (not with -g)\n" << usage;
        return 1;
    }
    if (trainer == Trainer::Softmax && (alpha_given || cg_given || gpus > 1 || sync_given || merge_given || weighting_given ||
                                        neighbours_given || l2_given || l1_given || sweeps_given)) {  // before the GPU is touched
        std::cerr << "mf: -m softmax takes no -a, -C, -W, -N, -L, -l or -n (its sweeps are the config's total_iterations), and is single-GPU only (no -g, -s, -w)\n"
                  << usage;
        return 1;
    }
    if ((weighting_given || neighbours_given) &&
        (trainer != Trainer::Knn || weighting < 0 || neighbours < 1 || neighbours > CU2REC_KNN_MAX_NEIGHBOURS)) {
        std::cerr << "mf: -W and -N need -m knn, a weighting of count, cosine, tfidf or bm25, and between 1 and " << CU2REC_KNN_MAX_NEIGHBOURS
                  << " neighbours\n" << usage;
        return 1;
    }
    if (trainer == Trainer::Lmf && !alpha_given) alpha = 1.f;
    if (takes_alpha && !(std::isfinite(alpha) && alpha >= 0.f)) {
        std::cerr << "mf: -a must be a finite number >= 0\n";
        return 1;
    }
    if (gpus > 1) {
        if (trainer != Trainer::Sgd) {
            std::cerr << "mf: -m " << trainer_name << " is single-GPU only (not with -g)\n";
            return 1;
        }
        if (mode == CU2REC_SGD_PINGPONG) {
            std::cerr << "mf: -m pingpong is single-GPU only\n";
            return 1;
        }
        return run_multi_gpu(gpus, mode, sync_every, merge, config_path, argv[optind], argv[optind + 1]);
    }
    try {
        if (cu2rec_device_count() < 1) throw std::runtime_error("no HIP device available");
        size_t free_bytes = 0, total_bytes = 0;  // mf.cu:33-37
        if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) throw std::runtime_error("hipMemGetInfo failed");
        std::printf("Free memory: %ld\n\n", static_cast<long>(free_bytes));

        const std::string train_path = argv[optind++];
        const cu2rec::HostCsr train = cu2rec::load_ratings(train_path);  // mf.cu:40-44
        const std::string test_path = argv[optind++];
        const cu2rec::HostCsr test = cu2rec::load_ratings(test_path);    // mf.cu:47-51
        if (train.nnz == 0) throw std::runtime_error("no ratings read from " + train_path);
        if (trainer == Trainer::Knn) return run_knn(train, test, train_path, weighting, static_cast<int>(neighbours), rank_k, rank_threshold);
        if (trainer == Trainer::Ease) return run_ease(train, test, train_path, l2, nullptr, rank_k, rank_threshold);
        if (is_slim) {
            const SlimOptions slim{l1, static_cast<int>(sweeps)};
            return run_ease(train, test, train_path, l2, &slim, rank_k, rank_threshold);
        }

        cu2rec_config cfg;  // mf.cu:54-57
        cu2rec::check(cu2rec_config_default(&cfg));
        if (!config_path.empty()) cu2rec::check(cu2rec_config_read(config_path.c_str(), &cfg));
        cu2rec::check(cu2rec_config_print(&cfg));
        mode = effective_mode(mode, cfg.n_factors);

        cu2rec::CsrHandle d_train(train), d_test(test);
        const float global_bias = trainer == Trainer::Svd ? 0.f : train.global_bias;  // PureSVD's scores are p . q
        cu2rec::ModelHandle model(train.rows, train.cols, cfg.n_factors, global_bias);
        std::vector<float> losses(static_cast<size_t>(cfg.total_iterations > 0 ? cfg.total_iterations : 1));
        if (trainer == Trainer::Svd)  // like -m ials: the test file is read, but only -k looks at it
            cu2rec::check(cu2rec_train_svd(d_train.h, &cfg, model.h, 1, nullptr));
        else if (trainer == Trainer::Bpr)  // like -m ials: the test file is read, but only -k looks at it
            cu2rec::check(cu2rec_train_bpr(d_train.h, &cfg, model.h, 1, nullptr, nullptr));
        else if (trainer == Trainer::Softmax)  // like -m ials: the test file is read, but only -k looks at it
            cu2rec::check(cu2rec_train_softmax(d_train.h, &cfg, model.h, 1, nullptr, nullptr));
        else if (trainer == Trainer::Lmf)
            cu2rec::check(cu2rec_train_lmf(d_train.h, &cfg, model.h, alpha, 1, nullptr, nullptr));
        else if (trainer == Trainer::Ials && cg_given)
            cu2rec::check(cu2rec_train_implicit_cg(d_train.h, &cfg, model.h, alpha, static_cast<int>(cg_steps), 1, nullptr, nullptr));
        else if (trainer == Trainer::Ials)  // the test file is read (and checked) as always, but only -k looks at it
            cu2rec::check(cu2rec_train_implicit(d_train.h, &cfg, model.h, alpha, 1, nullptr, nullptr));
        else if (trainer == Trainer::AlsCg)
            cu2rec::check(cu2rec_train_als_cg(d_train.h, d_test.h, &cfg, model.h, static_cast<int>(cg_steps), 1, losses.data(), nullptr));
        else  // an SGD mode, or Trainer::Als as CU2REC_ALS
            cu2rec::check(cu2rec_train(d_train.h, d_test.h, &cfg, model.h, mode, 1, losses.data(), nullptr));  // mf.cu:61

        std::vector<float> P(static_cast<size_t>(train.rows) * cfg.n_factors), Q(static_cast<size_t>(train.cols) * cfg.n_factors);
        std::vector<float> user_bias(train.rows), item_bias(train.cols);
        cu2rec::check(cu2rec_model_download(model.h, P.data(), Q.data(), user_bias.data(), item_bias.data()));

        // mf.cu:65-87: outputs go next to the training file, named <base>_f<F>_<component>.csv
        std::string parent_dir, base;
        output_place(train_path, parent_dir, base);
        const float gb = global_bias;
        const int f = cfg.n_factors;
        cu2rec::check(cu2rec_write_component(parent_dir.c_str(), base.c_str(), "p", P.data(), train.rows, f, f));
        cu2rec::check(cu2rec_write_component(parent_dir.c_str(), base.c_str(), "q", Q.data(), train.cols, f, f));
        cu2rec::check(cu2rec_write_component(parent_dir.c_str(), base.c_str(), "user_bias", user_bias.data(), train.rows, 1, f));
        cu2rec::check(cu2rec_write_component(parent_dir.c_str(), base.c_str(), "item_bias", item_bias.data(), train.cols, 1, f));
        cu2rec::check(cu2rec_write_component(parent_dir.c_str(), base.c_str(), "global_bias", &gb, 1, 1, f));
        if (rank_given) {  // the trained model ranks every user's unrated items against the test file
            cu2rec_rank_metrics rm;
            cu2rec::check(cu2rec_model_rank_metrics(model.h, d_train.h, d_test.h, rank_k, rank_threshold, &rm, nullptr));
            print_rank_line(rm, rank_k);
        }
    } catch (const std::exception &e) {
        std::cerr << "mf: " << e.what() << "\n";
        return 2;
    }
    return 0;
}
