// bin/predict -- partial fit for new users against a trained model, then recommendations.
// Drop-in for the reference CLI (predict.cu:72-146):
//
//   bin/predict -c config -i item_bias.csv -g global_bias.csv -q q.csv [-u] [-A] [-I alpha] [-P] [-k K] user_ratings.csv
//
// Q, item_bias and global_bias come from the files bin/mf wrote; only the users' factor rows and biases are
// trained (is_train = false).  Unlike the reference, the frozen-item flag really reaches the device (there
// `set_cuda_variables` never uploads is_train, config.cu:24-35, so its Q keeps moving).  The list of items to
// recommend is "every item the user has not rated", whatever order the ratings file is in (the reference
// assumes item-sorted ratings and dereferences end(), predict.cu:49-63).
// Default = the reference: EVERY record of the file belongs to the one new user, whatever its userId column says
// (predict.cu:119-121).  -u: a file of MANY users -- each distinct userId is a new user of its own; all of them are
// fitted in one batch (frozen items: no update crosses users, so every fit equals the one-user result), scored with one
// dense product on the matrix cores and ranked by one segmented sort on the device (cu2rec_model_scores /
// cu2rec_model_recommend); output is one block per user, headed "User: <id>".  -k K limits the recommendations listed.
//
// -A: the new users are fitted by ONE exact alternating-least-squares user half-step against the frozen item side
// (cu2rec_model_als, the config's P_reg and user_bias_reg) instead of the SGD loop: the optimum of each user's regularised
// objective in one call.  Works with and without -u; scoring, ranking and output are unchanged.
//
// -I alpha: the implicit-feedback fold-in for a model trained by bin/mf -m ials -- ONE implicit user half-step against the frozen
// q.csv (cu2rec_model_als_implicit with confidence weight alpha * r and the config's P_reg; every item of q.csv counts, the
// file's items as positives).  Not together with -A.
//
// -P: the fold-in for a model built by bin/mf -m svd -- no fit at all, the new users' rows are the projection p = r Q of their
// ratings on the frozen q.csv (cu2rec_model_project), their biases 0.  Not together with -A or -I.
//
//   bin/predict -c config -q q.csv -S [-k K] item_ids.txt
//
// -S fits no user: for each 0-based item index of the file (one per line, the numbers the "Item:" lines print) it lists the
// K (default 10) items whose rows of Q are nearest by cosine (cu2rec_model_similar), the item itself never among them.
#include <getopt.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <utility>
#include <vector>

#include "cu2rec.hpp"

namespace {

struct FloatTable {
    float *data = nullptr;
    int rows = 0, cols = 0;
    explicit FloatTable(const std::string &path) { cu2rec::check(cu2rec_read_array(path.c_str(), &data, &rows, &cols)); }
    FloatTable(const FloatTable &) = delete;
    FloatTable &operator=(const FloatTable &) = delete;
    ~FloatTable() { cu2rec_free(data); }
};

// -S: one 0-based item index per line (blank lines skipped)
std::vector<int> read_ids(const std::string &path) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error("cannot open " + path);
    std::vector<int> ids;
    std::string line;
    for (int no = 1; std::getline(in, line); ++no) {
        const size_t b = line.find_first_not_of(" \t\r"), e = line.find_last_not_of(" \t\r");
        if (b == std::string::npos) continue;
        const std::string t = line.substr(b, e - b + 1);
        size_t used = 0;
        long v = -1;
        try {
            v = std::stol(t, &used);
        } catch (const std::exception &) {
            used = 0;
        }
        if (used != t.size() || v < 0 || v > 0x7FFFFFFF) throw std::runtime_error(path + ":" + std::to_string(no) + ": not an item index: " + t);
        ids.push_back(static_cast<int>(v));
    }
    return ids;
}

// the cosine-nearest items of each listed item, from Q alone
int similar_items(const cu2rec_config &cfg, const std::string &q_path, const std::string &ids_path, int k) {
    const FloatTable Q(q_path);
    const int n_items = Q.rows, f = cfg.n_factors;
    if (n_items <= 0 || Q.cols != f) throw std::runtime_error("q file does not have n_factors columns");
    const std::vector<int> ids = read_ids(ids_path);
    for (int id : ids)
        if (id >= n_items) throw std::runtime_error("item index " + std::to_string(id) + " is not below the model's " + std::to_string(n_items) + " items");
    const std::vector<float> p(f, 0.f), ub(1, 0.f), ib(n_items, 0.f);  // no user is fitted; biases do not enter cosine
    cu2rec::ModelHandle model(1, n_items, f, 0.f, p.data(), Q.data, ub.data(), ib.data());
    const int n = static_cast<int>(ids.size());
    std::vector<int> near(static_cast<size_t>(n) * k);
    std::vector<float> cosine(static_cast<size_t>(n) * k);
    if (n > 0)
        cu2rec::check(cu2rec_model_similar(model.h, CU2REC_SIDE_ITEMS, CU2REC_SIM_COSINE, nullptr, ids.data(), n, k, near.data(),
                                           cosine.data()));
    for (int q = 0; q < n; ++q) {
        std::cout << "Item: " << ids[q] << "\n" << "Similar items:" << "\n";
        for (int j = 0; j < k; ++j) {
            const int item = near[static_cast<size_t>(q) * k + j];
            if (item < 0) break;
            std::printf("Rank: %d\tItem: %d\tCosine similarity: %f\n", j + 1, item, cosine[static_cast<size_t>(q) * k + j]);
        }
        std::fflush(stdout);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;  // predict.cu:73-75
    std::string config_path, item_bias_path, global_bias_path, q_path;
    bool many_users = false, similar = false, als = false, implicit = false, projection = false;
    float alpha = 0.f;  // -I
    int top_k = 0;  // 0: every unrated item, as the reference prints
    const char *k_arg = nullptr;
    int opt;
    while ((opt = getopt(argc, argv, "c:i:g:q:uk:SAI:P")) != -1) {
        switch (opt) {
            case 'u': many_users = true; break;
            case 'S': similar = true; break;
            case 'A': als = true; break;
            case 'P': projection = true; break;
            case 'I': {
                char *end = nullptr;
                implicit = true;
                alpha = std::strtof(optarg, &end);
                if (end == optarg || *end != '\0') alpha = NAN;  // not a number: refused below
                break;
            }
            case 'k':
                top_k = std::max(0, std::atoi(optarg));
                k_arg = optarg;
                break;
            case 'c': config_path = optarg; break;
            case 'i': item_bias_path = optarg; break;
            case 'g': global_bias_path = optarg; break;
            case 'q': q_path = optarg; break;
            default:
                std::cout << "Unknown option.\n";  // predict.cu:96-98
                return 1;
        }
    }
    if (similar) {
        const char *usage = "usage: predict -c config -q q.csv -S [-k K] item_ids.txt   (1 <= K <= 256; -S fits no user: no -u)\n";
        char *end = nullptr;
        const long k = k_arg ? std::strtol(k_arg, &end, 10) : 10;
        if (optind + 1 != argc || config_path.empty() || q_path.empty() || many_users || (k_arg && (*end || end == k_arg)) || k < 1 ||
            k > 256) {
            std::cerr << usage;
            return 2;
        }
        try {
            cu2rec_config cfg;
            cu2rec::check(cu2rec_config_default(&cfg));
            cu2rec::check(cu2rec_config_read(config_path.c_str(), &cfg));
            return similar_items(cfg, q_path, argv[optind], static_cast<int>(k));
        } catch (const std::exception &e) {
            std::cerr << "predict: " << e.what() << "\n";
            return 3;
        }
    }
    if (projection && (als || implicit)) {
        std::cerr << "predict: -P excludes -A and -I\n";
        return 2;
    }
    if (optind >= argc || config_path.empty() || item_bias_path.empty() || global_bias_path.empty() || q_path.empty()) {
        std::cerr << "usage: predict -c config -i item_bias.csv -g global_bias.csv -q q.csv [-u] [-A] [-I alpha] [-P] [-k K] user_ratings.csv\n";
        return 2;
    }
    if (als && implicit) {
        std::cerr << "predict: -A and -I exclude each other\n";
        return 2;
    }
    if (implicit && !(std::isfinite(alpha) && alpha >= 0.f)) {
        std::cerr << "predict: -I must be a finite number >= 0\n";
        return 2;
    }
    try {
        cu2rec_config cfg;
        cu2rec::check(cu2rec_config_default(&cfg));
        cu2rec::check(cu2rec_config_read(config_path.c_str(), &cfg));  // predict.cu:103-104
        cfg.is_train = 0;                                               // predict.cu:105

        const FloatTable item_bias(item_bias_path), gb(global_bias_path), Q(q_path);  // predict.cu:110-113
        const int n_items = Q.rows;
        if (n_items <= 0 || Q.cols != cfg.n_factors) throw std::runtime_error("q file does not have n_factors columns");
        if (item_bias.rows * item_bias.cols != n_items) throw std::runtime_error("item_bias and q disagree on the item count");
        if (gb.rows * gb.cols < 1) throw std::runtime_error("empty global_bias file");
        const float global_bias = gb.data[0];

        // the ratings: every record becomes user 0 (predict.cu:117-123), or with -u one new user per distinct userId.
        // Read as raw records: the file need not be sorted by user, and its userId column need not start at 1.
        cu2rec_ratings *raw = nullptr;
        cu2rec::check(cu2rec_ratings_read_csv(argv[optind], &raw));
        int n = 0, file_rows = 0, file_cols = 0;
        float file_gb = 0.f;
        const int *ru = nullptr, *ri = nullptr;
        const float *rr = nullptr;
        cu2rec::check(cu2rec_ratings_info(raw, &n, &file_rows, &file_cols, &file_gb));
        cu2rec::check(cu2rec_ratings_view(raw, &ru, &ri, &rr));
        if (file_cols > n_items) throw std::runtime_error("user ratings name an item the model does not have");
        std::vector<int> order(n);
        for (int k = 0; k < n; ++k) order[k] = k;
        std::vector<int> user_ids;  // 1-based ids as in the file, one per new user
        if (many_users) {
            std::stable_sort(order.begin(), order.end(), [&](int l, int r) { return ru[l] < ru[r]; });
            for (int k = 0; k < n; ++k)
                if (user_ids.empty() || user_ids.back() != ru[order[k]] + 1) user_ids.push_back(ru[order[k]] + 1);
        } else {
            user_ids.push_back(1);
        }
        cu2rec::HostCsr users;
        users.rows = static_cast<int>(user_ids.size());
        users.cols = n_items;
        users.nnz = n;
        users.indptr.assign(1, 0);
        for (int k = 0; k < n; ++k) {
            if (many_users && k > 0 && ru[order[k]] != ru[order[k - 1]]) users.indptr.push_back(k);
            users.indices.push_back(ri[order[k]]);
            users.data.push_back(rr[order[k]]);
        }
        users.indptr.push_back(n);
        cu2rec_ratings_free(raw);
        if (static_cast<int>(users.indptr.size()) != users.rows + 1) throw std::runtime_error("internal: bad user grouping");

        cu2rec::CsrHandle d_users(users);
        // every new user starts from the reference's seed-42 draw of ONE user (training.cu:28,54): the same prefix
        const int B = users.rows, f = cfg.n_factors;
        std::vector<float> P0(static_cast<size_t>(B) * f), ub0(B), one_p(f), one_ub(1);
        cu2rec::check(cu2rec_init_normal(one_p.data(), one_p.size(), f, 0.f, 1.f, 42));
        cu2rec::check(cu2rec_init_normal(one_ub.data(), 1, f, 0.f, 1.f, 42));
        for (int u = 0; u < B; ++u) {
            std::copy(one_p.begin(), one_p.end(), P0.begin() + static_cast<size_t>(u) * f);
            ub0[u] = one_ub[0];
        }
        if (projection) {  // p = r Q through a first model, of which only Q is read; the users' biases are 0
            cu2rec::ModelHandle items_only(B, n_items, f, global_bias, P0.data(), Q.data, ub0.data(), item_bias.data);
            cu2rec::check(cu2rec_model_project(items_only.h, d_users.h, P0.data()));
            std::fill(ub0.begin(), ub0.end(), 0.f);
        }
        cu2rec::ModelHandle model(B, n_items, f, global_bias, P0.data(), Q.data, ub0.data(), item_bias.data);
        if (projection) {
            // nothing is fitted
        } else if (als || implicit) {  // one exact user half-step: every user's optimum against the frozen items
            const cu2rec_hyper h{cfg.learning_rate, cfg.P_reg, cfg.Q_reg, cfg.user_bias_reg, cfg.item_bias_reg};
            int unsolved = 0;
            cu2rec::check(implicit ? cu2rec_model_als_implicit(model.h, d_users.h, &h, alpha, CU2REC_SIDE_USERS, &unsolved)
                                   : cu2rec_model_als(model.h, d_users.h, &h, CU2REC_SIDE_USERS, &unsolved));
            if (unsolved) std::cerr << "predict: " << unsolved << " user(s) could not be fitted (non-finite values); they keep the initial factors\n";
        } else {
            std::vector<float> losses(static_cast<size_t>(cfg.total_iterations > 0 ? cfg.total_iterations : 1));
            // frozen items: no two updates can conflict, every mode gives the sequential result; Hogwild runs all of a call's
            // iterations for all users in one launch
            cu2rec::check(cu2rec_train(d_users.h, d_users.h, &cfg, model.h, B == 1 ? CU2REC_SGD_SERIAL : CU2REC_SGD_HOGWILD, 1,
                                       losses.data(), nullptr));  // predict.cu:126
        }

        // predict_ratings (predict.cu:18-30) and get_recommendations (predict.cu:50-65), on the device
        std::vector<float> predictions(static_cast<size_t>(B) * n_items);
        cu2rec::check(cu2rec_model_scores_host(model.h, predictions.data()));
        const int k_list = top_k > 0 ? std::min(top_k, n_items) : n_items;
        std::vector<int> rec_items(static_cast<size_t>(B) * k_list);
        std::vector<float> rec_scores(static_cast<size_t>(B) * k_list);
        cu2rec::check(cu2rec_model_recommend(model.h, d_users.h, k_list, rec_items.data(), rec_scores.data()));
        for (int u = 0; u < B; ++u) {
            if (many_users) std::cout << "User: " << user_ids[u] << "\n";
            std::cout << "Predictions: " << "\n" << "[";  // print_predictions, predict.cu:32-39
            for (int i = 0; i < n_items; ++i) std::cout << predictions[static_cast<size_t>(u) * n_items + i] << ", ";
            std::cout << "]\n";
            std::cout << "Recommendations:" << std::endl;  // print_recommendations, predict.cu:67-72
            for (int j = 0; j < k_list; ++j) {
                const int item = rec_items[static_cast<size_t>(u) * k_list + j];
                if (item < 0) break;
                std::printf("Rank: %d\tItem: %d\tEstimated rating: %f\n", j + 1, item, rec_scores[static_cast<size_t>(u) * k_list + j]);
            }
        }
    } catch (const std::exception &e) {
        std::cerr << "predict: " << e.what() << "\n";
        return 3;
    }
    return 0;
}
