// commit_batch_driver.cpp — CommitBatch (tokamak-zk-evm_amd/host/tkmk_host.hpp) on two loopback ranks: one batch that holds the same
// REPLICATED polynomial twice, a second replicated polynomial and one whose box leaves rank 1 empty — every job's slice of a
// replicated polynomial is the batch's own — run in line and again through the helper-thread handle, next to the world-1 commits over
// the whole grid.  Inputs written and results compared by tests/test_gpu_commit_batch.py.
//   in : u32 rs_x, rs_y, then (xs, ys) of P, Q, S | crs[rs_x*rs_y] (96 B each) | P | Q | S coefficients
//   out: records { u32 tag, u64 nbytes, payload }: 1 = encode_poly of P, Q, S over the whole grid; 10 + r = rank r's batch [P, P, Q, S]
//        run in line; 20 + r = the same batch through CommitBatch::start
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "tkmk_host.hpp"

using namespace tkmk;

template <class T>
static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
    return v;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    auto emit = [&](uint32_t tag, const std::vector<G1Affine> &v) {
        const uint64_t n = v.size() * sizeof(G1Affine);
        fwrite(&tag, 4, 1, out), fwrite(&n, 8, 1, out), fwrite(v.data(), 1, n, out);
    };
    constexpr int G = 2;
    try {
        check(tkmk_set_device(0), "set_device");
        auto h = rd<uint32_t>(in, 8);
        const size_t rs_x = h[0], rs_y = h[1];
        auto crs = rd<G1Affine>(in, rs_x * rs_y);
        std::vector<ScalarField> coeffs[3];
        for (int k = 0; k < 3; k++) coeffs[k] = rd<ScalarField>(in, (size_t)h[2 + 2 * k] * h[3 + 2 * k]);
        auto poly = [&](int k) { return DensePolynomialExt::from_coeffs(coeffs[k], h[2 + 2 * k], h[3 + 2 * k]); };   // host values: replicated
        const DeviceVec<G1Affine> grid = DeviceVec<G1Affine>::from_host(crs);
        {
            Sigma1 whole(grid.clone(), rs_x, rs_y);
            std::vector<G1Affine> one_gpu;
            for (int k = 0; k < 3; k++) {
                DensePolynomialExt p = poly(k);
                one_gpu.push_back(whole.encode_poly(p));
            }
            emit(1, one_gpu);
        }
        check(tkmk_device_synchronize(), "synchronize");

        void *dist = dlopen("libtkmk_dist.so", RTLD_NOW);   // by the driver's run path; ShardLink::resolve then finds it loaded
        auto init_loopback = dist ? (decltype(&tkmk_comm_init_loopback))dlsym(dist, "tkmk_comm_init_loopback") : nullptr;
        auto destroy = dist ? (decltype(&tkmk_comm_destroy))dlsym(dist, "tkmk_comm_destroy") : nullptr;
        if (!init_loopback || !destroy) throw Error("libtkmk_dist.so not found");
        tkmk_comm *comms[G];
        check(init_loopback(G, comms), "tkmk_comm_init_loopback");
        std::vector<G1Affine> in_line[G], by_helper[G];
        std::string failed[G];
        auto rank_main = [&](int r) {
            ShardLink link;
            try {
                check(tkmk_set_device(0), "set_device");
                link = ShardLink::resolve(comms[r]);
                ShardSpan span(link);
                const Sigma1 sigma(Sigma1::cols_of_grid(grid, rs_x, rs_y, link.shard), rs_x, rs_y, 0, link.shard);
                const DensePolynomialExt P = poly(0), Q = poly(1), S = poly(2);
                auto batch_of = [&] {
                    CommitBatch b;
                    sigma.job(b, P, "P"), sigma.job(b, P, "P"), sigma.job(b, Q, "Q"), sigma.job(b, S, "S");
                    return b;
                };
                in_line[r] = batch_of().run();
                CommitBatch again = batch_of();
                tkmk_stream st = nullptr;
                check(tkmk_stream_create(&st), "stream_create");
                check(tkmk_device_synchronize(), "synchronize");   // the slices are cut: the helper's stream may read them
                // the helper issues this rank's device work now: it takes the device turn itself, entry by entry
                check(link.device_turn(link.comm, 0), "tkmk_comm_device_turn");
                try {
                    by_helper[r] = std::move(again).start(st).get();
                } catch (...) {
                    (void)link.device_turn(link.comm, 1);
                    throw;
                }
                check(link.device_turn(link.comm, 1), "tkmk_comm_device_turn");
                check(tkmk_stream_destroy(st), "stream_destroy");
            } catch (const std::exception &ex) {
                failed[r] = ex.what();
                if (link) (void)link.abort(link.comm);   // the peer fails in its next collective instead of waiting
            }
        };
        std::thread t1(rank_main, 1);
        rank_main(0);
        t1.join();
        for (int r = 0; r < G; r++) (void)destroy(comms[r]);
        for (int r = 0; r < G; r++)
            if (!failed[r].empty()) throw Error("rank " + std::to_string(r) + ": " + failed[r]);
        for (int r = 0; r < G; r++) emit(10 + r, in_line[r]), emit(20 + r, by_helper[r]);
    } catch (const std::exception &ex) {
        fprintf(stderr, "commit_batch_driver: %s\n", ex.what());
        return 1;
    }
    fclose(out);
    return 0;
}
