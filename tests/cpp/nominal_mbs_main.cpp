// mvtv::mbs_impl with mbs_impl_options::nominal on a mesh the reference rule refuses (tests/test_gpu_cxx_nominal.py).
// Input and output files as multivartv_amd/csrc/mvtv_mbs_cli.cpp reads and writes them; argv[3] = "batched" runs the
// CV as one mvtv_cv_batch call. Prints "refused <status>" for the default options' mvtv_error first.
#include <cstdint>
#include <cstdio>
#include <string>

#include "mvtv/solvers.hpp"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int64_t hdr[7];
    if (std::fread(hdr, sizeof(int64_t), 7, in) != 7) return 2;
    const int64_t n = hdr[0], p = hdr[1], nl = hdr[2], folds = hdr[3], seed = hdr[4], given = hdr[5];
    mvtv::vec m(static_cast<size_t>(p)), y(static_cast<size_t>(n)), lambdas(static_cast<size_t>(given ? nl : 0));
    mvtv::mat data(n, p);
    if (std::fread(m.data(), 8, m.size(), in) != m.size() ||
        std::fread(data.v.data(), 8, data.v.size(), in) != data.v.size() ||
        std::fread(y.data(), 8, y.size(), in) != y.size() ||
        std::fread(lambdas.data(), 8, lambdas.size(), in) != lambdas.size())
        return 2;
    std::fclose(in);
    try {
        (void)mvtv::mbs_impl(data, y, m, nullptr, int(nl), nullptr, given ? &lambdas : nullptr, int(folds), false,
                             uint64_t(seed));
        std::printf("accepted\n");
    } catch (const mvtv::mvtv_error& e) {
        std::printf("refused %d\n", e.status);
    }
    mvtv::mbs_impl_options opt;
    opt.nominal = true;
    opt.batched = argc > 3 && std::string(argv[3]) == "batched";
    try {
        const auto R = mvtv::mbs_impl(data, y, m, nullptr, int(nl), nullptr, given ? &lambdas : nullptr, int(folds),
                                      false, uint64_t(seed), 0, &opt);
        std::FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 2;
        const int64_t oh[4] = {int64_t(R.lambdas.size()), R.lambda_minmse_ind, int64_t(R.best.theta_hat.size()), n};
        std::fwrite(oh, 8, 4, out);
        std::fwrite(R.lambdas.data(), 8, R.lambdas.size(), out);
        std::fwrite(R.cv_mses.data(), 8, R.cv_mses.size(), out);
        std::fwrite(R.final_path.mses.data(), 8, R.final_path.mses.size(), out);
        std::fwrite(R.best.theta_hat.data(), 8, R.best.theta_hat.size(), out);
        std::fwrite(R.best.fitted.data(), 8, R.best.fitted.size(), out);
        std::fwrite(R.residuals.data(), 8, R.residuals.size(), out);
        std::fclose(out);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "mbs_impl: %s\n", e.what());
        return 1;
    }
    return 0;
}
