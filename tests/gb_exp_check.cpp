// Host check of csrc/solver_gb_math.h (tests/test_gb_host.py): reads f64 values from the file argv[1], writes gb_exp and
// gb_expit of each to argv[2], so that the test can compare the C++ evaluation with NumPy's mirror bit for bit.
#include <cstdio>
#include <vector>

#include "../phenotypeseeker_amd/csrc/solver_gb_math.h"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<double> x;
    double v;
    while (fread(&v, sizeof v, 1, in) == 1) x.push_back(v);
    fclose(in);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 4;
    for (double a : x) {
        const double r[2] = {gb_exp(a), gb_expit(a)};
        if (fwrite(r, sizeof r, 1, out) != 1) return 5;
    }
    return fclose(out) == 0 ? 0 : 6;
}
