// lm_core.h on the host, under the address and undefined-behaviour sanitizers (tests/test_lm_core_host_sanitized.py).
//
// Two drivers consume the same scripted trials (solved?, chi2 of the trial state, computeScale()):
//   * g2o_levenberg: a literal restatement of OptimizationAlgorithmLevenberg::solve and computeLambdaInit
//     (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:85-161, :166-180), members and all, with the spelling of the cube as
//     a parameter;
//   * composed: the lm_core.h functions put together the way a solver loop of the library puts them together.
// After every trial lambda, ni, the current chi2, qmax, nBad, "another trial" and "stop" must be equal bit for bit, for both spellings of
// the cube. How often the two spellings give different good-step factors is printed, not asserted.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "lm_core.h"

using namespace viorb;

struct Trial { bool solved; double chi; double scale; bool relative; };     // relative: chi is a factor on the chi2 of the state before the trial
struct Script { double chi0, max_diag; std::vector<std::vector<Trial>> iterations; };   // ten trials per iteration are enough for any run
struct Snap { double lambda, ni, chi; int qmax, nBad; bool again, stop; };
typedef double (*cube_fn)(double);
static double cube_pow(double t) { return pow(t, 3); }
static double cube_mul(double t) { return t * t * t; }

// the optimizer the algorithm drives: a state whose chi2 the script dictates, with push / pop
struct Graph {
    double chi, saved = 0;
    void push() { saved = chi; }
    void pop() { chi = saved; }
    double trial(const Trial& t) { chi = t.relative ? chi * t.chi : t.chi; return chi; }      // update() + computeActiveErrors() + activeRobustChi2()
};

struct g2o_levenberg {
    double _currentLambda = -1., _tau = 1e-5, _goodStepUpperScale = 2. / 3., _goodStepLowerScale = 1. / 3., _ni = 2.;
    int _maxTrialsAfterFailure = 10, _levenbergIterations = 0, _nBad = 0;
    enum Result { OK, Terminate };
    double computeLambdaInit(double maxDiagonal) const { return _tau * maxDiagonal; }
    Result solve(int iteration, Graph& g, double max_diag, const std::vector<Trial>& trials, cube_fn cube, std::vector<Snap>& out) {
        double currentChi = g.chi;
        double tempChi = currentChi;
        double iniChi = currentChi;
        if (iteration == 0) {
            _currentLambda = computeLambdaInit(max_diag);
            _ni = 2;
            _nBad = 0;
        }
        double rho = 0;
        int& qmax = _levenbergIterations;
        qmax = 0;
        bool again;
        do {
            g.push();
            const Trial& t = trials.at(qmax);
            bool ok2 = t.solved;
            tempChi = g.trial(t);
            if (!ok2)
                tempChi = std::numeric_limits<double>::max();
            rho = (currentChi - tempChi);
            double scale = t.scale;                        // computeScale()
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - cube(2 * rho - 1);
                alpha = (std::min)(alpha, _goodStepUpperScale);
                double scaleFactor = (std::max)(_goodStepLowerScale, alpha);
                _currentLambda *= scaleFactor;
                _ni = 2;
                currentChi = tempChi;
            } else {
                _currentLambda *= _ni;
                _ni *= 2;
                g.pop();
            }
            qmax++;
            again = rho < 0 && qmax < _maxTrialsAfterFailure;
            if (again) out.push_back(Snap{_currentLambda, _ni, currentChi, qmax, _nBad, true, false});
        } while (again);
        Result r = OK;
        if (qmax == _maxTrialsAfterFailure || rho == 0)
            r = Terminate;
        else {
            if ((iniChi - currentChi) * 1e3 < iniChi)
                _nBad++;
            else
                _nBad = 0;
            if (_nBad >= 3)
                r = Terminate;
        }
        out.push_back(Snap{_currentLambda, _ni, currentChi, qmax, _nBad, false, r == Terminate});
        return r;
    }
};

static std::vector<Snap> run_reference(const Script& s, cube_fn cube) {
    std::vector<Snap> out;
    g2o_levenberg alg; Graph g{s.chi0};
    for (size_t it = 0; it < s.iterations.size(); it++)
        if (alg.solve((int)it, g, s.max_diag, s.iterations[it], cube, out) == g2o_levenberg::Terminate) break;
    return out;
}

// the shape of k_pose_opt_se3 / k_sim3_optimize / gba_run: state in plain variables, the rule from lm_core.h
template <bool POW> static std::vector<Snap> run_composed(const Script& s, long* accepted, long* factor_differs) {
    std::vector<Snap> out;
    Graph g{s.chi0};
    double lambda = -1., ni = 2; int nBad = 0;
    for (size_t it = 0; it < s.iterations.size(); it++) {
        double currentChi = g.chi;
        const double iniChi = currentChi;
        if (it == 0) { lambda = lm_lambda_init(s.max_diag); ni = 2; nBad = 0; }
        double rho = 0; int qmax = 0;
        bool again;
        do {
            g.push();
            const Trial& t = s.iterations[it].at(qmax);
            const double tempChi = lm_trial_chi2(t.solved, g.trial(t));
            rho = lm_rho(currentChi, tempChi, t.scale);
            if (lm_accepted(rho, tempChi)) {
                double l1 = 1, l2 = 1, n1, n2;
                lm_good_step(l1, n1, lm_cube_pow(2 * rho - 1)); lm_good_step(l2, n2, lm_cube_mul(2 * rho - 1));
                ++*accepted; if (l1 != l2) ++*factor_differs;
                lm_good_step(lambda, ni, POW ? lm_cube_pow(2 * rho - 1) : lm_cube_mul(2 * rho - 1)); currentChi = tempChi;
            } else { lm_bad_step(lambda, ni); g.pop(); }
            qmax++;
            again = lm_retry(rho, qmax);
            if (again) out.push_back(Snap{lambda, ni, currentChi, qmax, nBad, true, false});
        } while (again);
        const bool stop = lm_iteration_stops(rho, qmax, iniChi, currentChi, nBad);
        out.push_back(Snap{lambda, ni, currentChi, qmax, nBad, false, stop});
        if (stop) break;
    }
    return out;
}

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { failures++; printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } while (0)
static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }
static bool same(const Snap& a, const Snap& b) {
    return same_bits(a.lambda, b.lambda) && same_bits(a.ni, b.ni) && same_bits(a.chi, b.chi) && a.qmax == b.qmax && a.nBad == b.nBad && a.again == b.again && a.stop == b.stop;
}
static long n_accepted = 0, n_differs = 0, n_trials = 0, n_stops = 0;
// both spellings, reference against composed, after every trial; returns the composed run with the pow spelling
static std::vector<Snap> check(const char* name, const Script& s) {
    std::vector<Snap> keep;
    for (int spelling = 0; spelling < 2; spelling++) {
        long acc = 0, dif = 0;
        const std::vector<Snap> ref = run_reference(s, spelling == 0 ? cube_pow : cube_mul);
        const std::vector<Snap> got = spelling == 0 ? run_composed<true>(s, &acc, &dif) : run_composed<false>(s, &acc, &dif);
        CHECK(ref.size() == got.size(), "%s spelling %d: %zu trials against %zu", name, spelling, ref.size(), got.size());
        for (size_t i = 0; i < ref.size() && i < got.size(); i++)
            CHECK(same(ref[i], got[i]), "%s spelling %d trial %zu: lambda %.17g / %.17g ni %g / %g chi %.17g / %.17g qmax %d / %d nBad %d / %d again %d / %d stop %d / %d", name, spelling, i,
                  ref[i].lambda, got[i].lambda, ref[i].ni, got[i].ni, ref[i].chi, got[i].chi, ref[i].qmax, got[i].qmax, ref[i].nBad, got[i].nBad, ref[i].again, got[i].again, ref[i].stop, got[i].stop);
        if (spelling == 0) { keep = got; n_accepted += acc; n_differs += dif; n_trials += (long)got.size(); n_stops += !got.empty() && got.back().stop; }
    }
    return keep;
}

static std::vector<Trial> one(bool solved, double chi, double scale) { return std::vector<Trial>(10, Trial{solved, chi, scale, false}); }

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double l0 = 1e-5 * 1000.0;
    // the good-step factor in its three regimes: rho = 1 -> 1 - 1 = 0 -> 1/3; rho = 0.9 -> 1 - 0.512 = 0.488; rho = 0.5 -> 1 -> 2/3
    // (scale + 1e-3 = 10 up to rounding, so rho is only close to these values: the clamped cases have margin, the middle one is an interval)
    {
        std::vector<Snap> r = check("factor clamped at 1/3", Script{100.0, 1000.0, {one(true, 90.0, 10.0 - 1e-3)}});
        CHECK(r.size() == 1 && same_bits(r[0].lambda, l0 * (1. / 3.)) && r[0].ni == 2 && r[0].chi == 90.0 && r[0].qmax == 1 && !r[0].stop, "lambda %.17g", r[0].lambda);
        r = check("factor in between", Script{100.0, 1000.0, {one(true, 91.0, 10.0 - 1e-3)}});
        CHECK(r.size() == 1 && r[0].lambda > l0 * 0.48 && r[0].lambda < l0 * 0.50, "lambda %.17g", r[0].lambda);
        r = check("factor clamped at 2/3", Script{100.0, 1000.0, {one(true, 95.0, 10.0 - 1e-3)}});
        CHECK(r.size() == 1 && same_bits(r[0].lambda, l0 * (2. / 3.)), "lambda %.17g", r[0].lambda);
    }
    {   // rho == 0 exactly: the trial is rejected, not retried, and the optimisation stops
        std::vector<Snap> r = check("rho == 0", Script{100.0, 1000.0, {one(true, 100.0, 5.0), one(true, 50.0, 5.0)}});
        CHECK(r.size() == 1 && r[0].stop && !r[0].again && r[0].qmax == 1 && same_bits(r[0].lambda, l0 * 2) && r[0].ni == 4 && r[0].chi == 100.0 && r[0].nBad == 0, "size %zu", r.size());
    }
    {   // ten rejections in a row
        std::vector<Snap> r = check("qmax == 10", Script{100.0, 1000.0, {one(true, 150.0, 5.0), one(true, 50.0, 5.0)}});
        CHECK(r.size() == 10 && r[8].again && !r[9].again && r[9].stop && r[9].qmax == 10 && r[9].ni == 2048 && r[9].chi == 100.0, "size %zu", r.size());
        double l = l0, n = 2; for (int i = 0; i < 10; i++) { l *= n; n *= 2; }
        CHECK(same_bits(r[9].lambda, l), "lambda %.17g", r[9].lambda);
    }
    {   // a failed factorisation (a better chi2 that must not count), then a good trial of the same iteration
        std::vector<Trial> t = one(true, 60.0, 30.0); t[0] = Trial{false, 10.0, 7.0, false};
        std::vector<Snap> r = check("failed factorisation", Script{100.0, 1000.0, {t}});
        CHECK(r.size() == 2 && r[0].again && r[0].chi == 100.0 && r[0].ni == 4 && r[1].chi == 60.0 && r[1].qmax == 2 && !r[1].stop, "size %zu", r.size());
    }
    {   // inf: rho = -inf, retried; NaN: rho is NaN, neither retried nor a Terminate by the first test
        std::vector<Trial> t = one(true, 60.0, 30.0); t[0] = Trial{true, inf, 7.0, false};
        std::vector<Snap> r = check("trial chi2 inf", Script{100.0, 1000.0, {t}});
        CHECK(r.size() == 2 && r[0].again && r[1].chi == 60.0, "size %zu", r.size());
        t[0] = Trial{true, nan, 7.0, false};
        r = check("trial chi2 NaN", Script{100.0, 1000.0, {t, one(true, 60.0, 30.0)}});
        CHECK(r.size() == 2 && !r[0].again && !r[0].stop && r[0].qmax == 1 && r[0].nBad == 1 && r[0].chi == 100.0 && r[1].chi == 60.0 && r[1].nBad == 0, "size %zu", r.size());
    }
    {   // a negative scale with a worse chi2: rho > 0, accepted although chi2 went up
        std::vector<Snap> r = check("negative scale", Script{100.0, 1000.0, {one(true, 120.0, -40.0)}});
        CHECK(r.size() == 1 && r[0].chi == 120.0 && r[0].ni == 2 && r[0].nBad == 1, "size %zu", r.size());
    }
    {   // nBad reaching 3 over three iterations of negligible gain; a good iteration in between resets the count
        std::vector<Snap> r = check("nBad 3", Script{100.0, 1000.0, {one(true, 99.99, 1.0), one(true, 99.98, 1.0), one(true, 99.97, 1.0), one(true, 50.0, 100.0)}});
        CHECK(r.size() == 3 && r[0].nBad == 1 && r[1].nBad == 2 && !r[1].stop && r[2].nBad == 3 && r[2].stop, "size %zu", r.size());
        r = check("nBad reset", Script{100.0, 1000.0, {one(true, 99.99, 1.0), one(true, 99.98, 1.0), one(true, 50.0, 100.0), one(true, 49.999, 1.0), one(true, 49.998, 1.0), one(true, 49.997, 1.0), one(true, 1.0, 100.0)}});
        CHECK(r.size() == 6 && r[1].nBad == 2 && r[2].nBad == 0 && r[4].nBad == 2 && !r[4].stop && r[5].nBad == 3 && r[5].stop, "size %zu", r.size());
    }
    {   // iniChi == 0: an equal trial gives rho == 0; a NaN trial reaches the stall rule, where (0 - 0) * 1e3 < 0 is false
        std::vector<Snap> r = check("iniChi == 0, equal trial", Script{0.0, 1000.0, {one(true, 0.0, 1.0)}});
        CHECK(r.size() == 1 && r[0].stop && r[0].qmax == 1, "size %zu", r.size());
        r = check("iniChi == 0, NaN trial", Script{0.0, 1000.0, {one(true, nan, 1.0), one(true, nan, 1.0), one(true, nan, 1.0), one(true, nan, 1.0)}});
        CHECK(r.size() == 4 && r[3].nBad == 0 && !r[3].stop, "size %zu", r.size());
        r = check("iniChi == 0, worse trials", Script{0.0, 1000.0, {one(true, 1.0, 1.0)}});
        CHECK(r.size() == 10 && r[9].stop, "size %zu", r.size());
    }
    const long scripted = n_trials;
    // 10 000 seeded random scripts of up to 15 iterations: mostly improving trials around the accept / reject boundary, with stalls, equal
    // trials, failed solves, inf and NaN mixed in
    std::mt19937_64 rng(20240607u);
    auto uni = [&](double a, double b) { return a + (b - a) * (double)(rng() >> 11) * (1.0 / 9007199254740992.0); };
    for (int s = 0; s < 10000; s++) {
        Script sc; sc.chi0 = pow(10.0, uni(-2, 4)); sc.max_diag = pow(10.0, uni(-3, 6));
        if (s % 97 == 0) sc.chi0 = 0;
        const int its = 1 + (int)(rng() % 15);
        for (int it = 0; it < its; it++) {
            std::vector<Trial> t;
            for (int q = 0; q < 10; q++) {
                const double u = uni(0, 1), scale = sc.chi0 * uni(-0.2, 1.0);
                if (u < 0.03) t.push_back(Trial{false, uni(0.1, 1.0), scale, true});
                else if (u < 0.04) t.push_back(Trial{true, inf, scale, false});
                else if (u < 0.05) t.push_back(Trial{true, nan, scale, false});
                else if (u < 0.08) t.push_back(Trial{true, 1.0, scale, true});
                else if (u < 0.30) t.push_back(Trial{true, uni(0.9995, 1.0), scale, true});
                else if (u < 0.55) t.push_back(Trial{true, uni(1.0, 1.5), scale, true});
                else t.push_back(Trial{true, uni(0.2, 1.0), scale, true});
            }
            sc.iterations.push_back(t);
        }
        check("random", sc);
        if (failures > 20) break;
    }
    printf("lm_core: %ld scripted and %ld random trials compared, %ld runs ended by a stop rule; of %ld accepted trials the two spellings of the cube gave different factors in %ld\n",
           scripted, n_trials - scripted, n_stops, n_accepted, n_differs);
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("lm_core ok\n");
    return 0;
}
