// TEST INFRASTRUCTURE (tests/test_lin_noise_host.py): the staging of the resident loop's white noise, steps_to_soa of mpc-code_amd/csrc/mpc_host.hpp,
// exercised without a GPU - no HIP call is made.  Built with the host side under AddressSanitizer and UndefinedBehaviorSanitizer and run as a child
// process.  Host [nsteps][B][d] -> staging [step][d][Bs] with zero padding lanes, and back through LogTab::unpad, which reads that layout.
#include "mpc_host.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main()
{
    for (int B : {1, 63, 64, 65, 130})
        for (int d : {0, 2, 3})
            for (int n : {1, 3}) {
                const size_t Bs = pad64(B);
                std::vector<double> src((size_t)n * B * d), st((size_t)n * d * Bs, -7.0), back((size_t)n * B * d, -9.0);
                for (size_t i = 0; i < src.size(); i++) src[i] = 1.0 + (double)i;
                steps_to_soa(src.data(), n, B, d, Bs, st.data());
                for (int k = 0; k < n; k++)
                    for (int i = 0; i < d; i++) {
                        const double *row = st.data() + ((size_t)k * d + i) * Bs;      // what instance b reads as component i of step k: row[b]
                        for (int b = 0; b < B; b++) CHECK(row[b] == src[((size_t)k * B + b) * d + i]);
                        for (size_t b = B; b < Bs; b++) CHECK(row[b] == 0.0);          // the padding lanes
                    }
                LogTab::unpad(st.data(), n, d, B, Bs, back.data());
                CHECK(back == src);
            }
    std::printf("noise staging ok\n");
    return 0;
}
