// lm_core.h on the host, under the address and undefined-behaviour sanitizers (tests/test_lm_core_host_sanitized.py).
//
// Two drivers consume the same scripted trials (solved?, chi2 of the trial state, computeScale()):
//   * g2o_levenberg: a literal restatement of OptimizationAlgorithmLevenberg::solve and computeLambdaInit
//     (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:85-161, :166-180), members and all, with the spelling of the cube as
//     a parameter;
//   * composed: the lm_core.h functions put together the way a solver loop of the library puts them together.
// After every trial lambda, ni, the current chi2, qmax, nBad, "another trial" and "stop" must be equal bit for bit, for both spellings of
// the cube. How often the two spellings give different good-step factors is printed, not asserted.
//
// Then lba_ctl.h, the control block of the window solves: the restatement run over a window's two optimize() calls (with terminate())
// against a driver that keeps nothing but the 32-word block and calls lba_ctl_init / lba_lambda0 / lba_decide / lba_phase as the kernels
// of local_ba.hip do — after every trial the same seven values plus phase, iteration, trial and rejection counts, the chi2 of both
// calls and the gate, bit for bit; BA_B_QMAX == 0 at the start of every iteration and phase. Scripted: 5 + 10 accepted; reject, retry,
// accept; ten failed solves; stall stops in either call; nBad reset; the stop flag raised during an accepted and during a rejected
// trial; rejections in the last iteration of the second call. Then 2 000 seeded random windows.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "lba_ctl.h"

using namespace viorb;

struct Trial { bool solved; double chi; double scale; bool relative; bool abort = false; };     // relative: chi is a factor on the chi2 of the state before the trial; abort: the caller's stop flag goes up during this trial
struct Script { double chi0, max_diag; std::vector<std::vector<Trial>> iterations; };   // ten trials per iteration are enough for any run
struct Snap { double lambda, ni, chi; int qmax, nBad; bool again, stop, rejected; };
typedef double (*cube_fn)(double);
static double cube_pow(double t) { return pow(t, 3); }
static double cube_mul(double t) { return t * t * t; }

// the optimizer the algorithm drives: a state whose chi2 the script dictates, with push / pop
struct Graph {
    double chi, saved = 0;
    bool stop = false;                                                      // what terminate() returns
    void push() { saved = chi; }
    void pop() { chi = saved; }
    double trial(const Trial& t) { chi = t.relative ? chi * t.chi : t.chi; if (t.abort) stop = true; return chi; }      // update() + computeActiveErrors() + activeRobustChi2()
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
        bool again, rejected;
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
                rejected = false;
            } else {
                _currentLambda *= _ni;
                _ni *= 2;
                g.pop();
                rejected = true;
            }
            qmax++;
            again = rho < 0 && qmax < _maxTrialsAfterFailure && !g.stop;     // "&& ! _optimizer->terminate()"
            if (again) out.push_back(Snap{_currentLambda, _ni, currentChi, qmax, _nBad, true, false, rejected});
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
        out.push_back(Snap{_currentLambda, _ni, currentChi, qmax, _nBad, false, r == Terminate, rejected});
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
        bool again, rho_rejected;
        do {
            g.push();
            const Trial& t = s.iterations[it].at(qmax);
            const double tempChi = lm_trial_chi2(t.solved, g.trial(t));
            rho = lm_rho(currentChi, tempChi, t.scale);
            rho_rejected = !lm_accepted(rho, tempChi);
            if (lm_accepted(rho, tempChi)) {
                double l1 = 1, l2 = 1, n1, n2;
                lm_good_step(l1, n1, lm_cube_pow(2 * rho - 1)); lm_good_step(l2, n2, lm_cube_mul(2 * rho - 1));
                ++*accepted; if (l1 != l2) ++*factor_differs;
                lm_good_step(lambda, ni, POW ? lm_cube_pow(2 * rho - 1) : lm_cube_mul(2 * rho - 1)); currentChi = tempChi;
            } else { lm_bad_step(lambda, ni); g.pop(); }
            qmax++;
            again = lm_retry(rho, qmax);
            if (again) out.push_back(Snap{lambda, ni, currentChi, qmax, nBad, true, false, !lm_accepted(rho, tempChi)});
        } while (again);
        const bool stop = lm_iteration_stops(rho, qmax, iniChi, currentChi, nBad);
        out.push_back(Snap{lambda, ni, currentChi, qmax, nBad, false, stop, rho_rejected});
        if (stop) break;
    }
    return out;
}

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { failures++; printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } while (0)
static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }
static bool same(const Snap& a, const Snap& b) {
    return same_bits(a.lambda, b.lambda) && same_bits(a.ni, b.ni) && same_bits(a.chi, b.chi) && a.qmax == b.qmax && a.nBad == b.nBad && a.again == b.again && a.stop == b.stop && a.rejected == b.rejected;
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

// ---- lba_ctl.h: the control block of a window solve (local_ba.hip). A window is two optimize() calls, 5 and 10 iterations, the second
// only "if (!terminate())" (reference src/Optimizer.cc:2026-2099). The reference runs the restatement above over both; the driver below
// keeps nothing but the block and does around lba_lambda0 / lba_decide / lba_phase what the kernels of either driver do around them.
struct WScript { double chi0[2], max_diag[2]; std::vector<std::vector<Trial>> it[2]; };      // per optimize(): chi2 at its start, largest diagonal entry, iterations
struct WSnap { Snap s; int phase, its[2], trials, rejects; double chi[2], gate; };           // s.stop: this optimize() is over; gate: 1 second optimize() follows, 2 the window is finished

static std::vector<WSnap> window_reference(const WScript& w) {
    std::vector<WSnap> out;
    g2o_levenberg alg;                                     // one algorithm object for both calls, as in the reference: iteration 0 resets lambda, ni and nBad
    int its[2] = {0, 0}, trials = 0, rejects = 0; double chi[2] = {0, 0};
    bool stopped = false;
    for (int phase = 0; phase < 2 && !stopped; phase++) {
        Graph g{w.chi0[phase]};
        const int iters = phase == 0 ? 5 : 10;
        for (int it = 0; it < iters && !g.stop; it++) {
            std::vector<Snap> s;
            const bool term = alg.solve(it, g, w.max_diag[phase], w.it[phase].at(it), cube_mul, s) == g2o_levenberg::Terminate;
            for (size_t k = 0; k < s.size(); k++) {
                trials++; rejects += s[k].rejected;
                const bool last = k + 1 == s.size();
                if (last) { its[phase]++; chi[phase] = g.chi; }
                const bool over = last && (term || it + 1 == iters || g.stop);
                s[k].stop = over;
                out.push_back(WSnap{s[k], phase, {its[0], its[1]}, trials, rejects, {chi[0], chi[1]}, !over ? 0.0 : (g.stop || phase == 1) ? 2.0 : 1.0});
            }
            if (term) break;
        }
        stopped = g.stop;
    }
    return out;
}

static std::vector<WSnap> window_ctl(const char* name, const WScript& w) {
    std::vector<WSnap> out;
    double c[BA_B_N];
    for (int t = 0; t < BA_B_N; t++) c[t] = lba_ctl_init(t);
    do {
        const int phase = (int)c[BA_B_PHASE];
        CHECK(c[BA_B_QMAX] == 0.0 && c[BA_B_RESTORE] == 0.0 && c[BA_B_NEED_LIN] == 1.0 && c[BA_B_FIRST] == 1.0 && c[BA_CTL_IT] == 0.0, "%s: phase %d begins with qmax %g", name, phase, c[BA_B_QMAX]);
        Graph g{w.chi0[phase]};
        c[BA_CTL_CHI] = g.chi;                             // k_bab_take_chi / the first k_ba_clear_body of a phase
        while (c[BA_B_GATE] == 0.0) {
            if (c[BA_B_RESTORE] != 0.0) { g.pop(); c[BA_B_RESTORE] = 0.0; }                   // k_bab_restore + k_bab_phase / the retry slot's first launch + k_ba_f_errors_decide
            if (c[BA_B_NEED_LIN] != 0.0) {                 // a new iteration: linearise
                CHECK(c[BA_B_QMAX] == 0.0, "%s: iteration %g of phase %d begins with qmax %g", name, c[BA_CTL_IT], phase, c[BA_B_QMAX]);
                c[BA_CTL_INICHI] = c[BA_CTL_CHI];          // k_ba_clear_body
                if (c[BA_B_FIRST] != 0.0) lba_lambda0(c, w.max_diag[phase]);
                c[BA_B_NEED_LIN] = 0.0;                    // k_bab_lambda0 / k_ba_f_errors_decide
            }
            const int q = (int)c[BA_B_QMAX];
            const Trial& t = w.it[phase].at((size_t)c[BA_CTL_IT]).at(q);
            g.push();
            const double chi = g.trial(t);
            lba_decide(c, chi, t.scale, t.solved ? 1.0 : 0.0, t.abort);
            const bool again = c[BA_B_QMAX] != 0.0, over = c[BA_B_GATE] != 0.0;
            CHECK((int)again + (int)(c[BA_B_NEED_LIN] != 0.0) + (int)over == 1, "%s: retry %d, next iteration %g, gate %g", name, again, c[BA_B_NEED_LIN], c[BA_B_GATE]);
            out.push_back(WSnap{Snap{c[BA_CTL_LAMBDA], c[BA_CTL_NI], c[BA_CTL_CHI], again ? (int)c[BA_B_QMAX] : q + 1, (int)c[BA_CTL_NBAD], again, over, c[BA_B_RESTORE] != 0.0},
                                phase, {(int)c[BA_B_ITS0], (int)c[BA_B_ITS1]}, (int)c[BA_CTL_TRIALS], (int)c[BA_CTL_REJECTS], {c[BA_B_CHI0], c[BA_B_CHI1]}, c[BA_B_GATE]});
        }
        if (c[BA_B_RESTORE] != 0.0) g.pop();               // a rejection in the phase's last trial: restored before the gate
    } while (!lba_phase(c));
    CHECK(c[BA_B_DONE] == 1.0 && c[BA_B_GATE] == 0.0 && !lba_phase(c), "%s: done %g", name, c[BA_B_DONE]);
    return out;
}

static long n_window_trials = 0;
static std::vector<WSnap> check_window(const char* name, const WScript& w) {
    const std::vector<WSnap> ref = window_reference(w), got = window_ctl(name, w);
    CHECK(ref.size() == got.size(), "%s: %zu trials against %zu", name, ref.size(), got.size());
    for (size_t i = 0; i < ref.size() && i < got.size(); i++) {
        const WSnap &a = ref[i], &b = got[i];
        CHECK(same(a.s, b.s) && a.phase == b.phase && a.its[0] == b.its[0] && a.its[1] == b.its[1] && a.trials == b.trials && a.rejects == b.rejects &&
              same_bits(a.chi[0], b.chi[0]) && same_bits(a.chi[1], b.chi[1]) && a.gate == b.gate,
              "%s trial %zu: lambda %.17g / %.17g ni %g / %g chi %.17g / %.17g qmax %d / %d nBad %d / %d again %d / %d over %d / %d rejected %d / %d phase %d / %d its %d+%d / %d+%d trials %d / %d rejects %d / %d gate %g / %g",
              name, i, a.s.lambda, b.s.lambda, a.s.ni, b.s.ni, a.s.chi, b.s.chi, a.s.qmax, b.s.qmax, a.s.nBad, b.s.nBad, a.s.again, b.s.again, a.s.stop, b.s.stop, a.s.rejected, b.s.rejected,
              a.phase, b.phase, a.its[0], a.its[1], b.its[0], b.its[1], a.trials, b.trials, a.rejects, b.rejects, a.gate, b.gate);
    }
    n_window_trials += (long)got.size();
    return got;
}
// n iterations whose every trial multiplies chi2 by f (scale: a tenth of the chi2 the optimize() starts from)
static std::vector<std::vector<Trial>> steady(int n, double f, double chi0) { return std::vector<std::vector<Trial>>(n, std::vector<Trial>(10, Trial{true, f, 0.1 * chi0, true})); }

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
    // ---- the window's control block (lba_ctl.h) over two optimize() calls
    const Trial good{true, 0.5, 10.0, true}, worse{true, 1.5, 10.0, true}, stall{true, 0.99999, 10.0, true}, failed{false, 1.0, 0.0, true};
    auto plain = [&]() { return WScript{{100.0, 40.0}, {1000.0, 500.0}, {steady(5, 0.5, 100.0), steady(10, 0.5, 40.0)}}; };
    {
        std::vector<WSnap> r = check_window("5 + 10 accepted", plain());
        CHECK(r.size() == 15 && r[4].gate == 1.0 && r[4].its[0] == 5 && r[5].phase == 1 && r[14].gate == 2.0 && r[14].its[1] == 10 && r[14].trials == 15 && r[14].rejects == 0, "size %zu", r.size());
        CHECK(same_bits(r[5].s.lambda, 1e-5 * 500.0 * (1. / 3.)), "lambda_0 of the second optimize() comes from its own diagonal: %.17g", r[5].s.lambda);
    }
    {   // reject, retry, accept in the third iteration of the first optimize()
        WScript w = plain(); w.it[0][2] = {worse, worse, good, good, good, good, good, good, good, good};
        std::vector<WSnap> r = check_window("reject, retry, accept", w);
        CHECK(r.size() == 17 && r[2].s.again && r[2].s.rejected && r[2].s.qmax == 1 && r[3].s.again && r[3].s.qmax == 2 && !r[4].s.again && !r[4].s.rejected && r[4].s.qmax == 3 && r[4].its[0] == 3 &&
              r[16].trials == 17 && r[16].rejects == 2 && r[16].its[0] == 5 && r[16].its[1] == 10, "size %zu", r.size());
    }
    {   // ten failed solves in the first iteration of the second optimize(): Terminate on qmax == 10, chi2 unchanged
        WScript w = plain(); w.it[1][0] = std::vector<Trial>(10, failed);
        std::vector<WSnap> r = check_window("ten failed solves", w);
        CHECK(r.size() == 15 && r[13].s.again && r[13].s.qmax == 9 && !r[14].s.again && r[14].s.qmax == 10 && r[14].s.rejected && r[14].gate == 2.0 && r[14].its[1] == 1 && r[14].rejects == 10 &&
              same_bits(r[14].chi[1], 40.0), "size %zu", r.size());
    }
    {   // the stall rule ends the first optimize() after three iterations; the second one runs
        WScript w = plain(); w.it[0] = std::vector<std::vector<Trial>>(5, std::vector<Trial>(10, stall));
        std::vector<WSnap> r = check_window("stall stop, then the second optimize()", w);
        CHECK(r.size() == 13 && r[1].s.nBad == 2 && r[1].gate == 0.0 && r[2].s.nBad == 3 && r[2].gate == 1.0 && r[2].its[0] == 3 && r[3].phase == 1 && r[3].s.nBad == 0 && r[12].its[1] == 10, "size %zu", r.size());
        w = plain(); w.it[1] = std::vector<std::vector<Trial>>(10, std::vector<Trial>(10, stall));
        r = check_window("stall stop in the second optimize()", w);
        CHECK(r.size() == 8 && r[7].gate == 2.0 && r[7].its[1] == 3, "size %zu", r.size());
    }
    {   // nBad back to 0 between stalled iterations: ss.sss
        WScript w = plain();
        for (int i : {0, 1, 3, 4, 5}) w.it[1][i] = std::vector<Trial>(10, stall);
        std::vector<WSnap> r = check_window("nBad reset", w);
        CHECK(r.size() == 11 && r[6].s.nBad == 2 && r[7].s.nBad == 0 && r[9].s.nBad == 2 && r[10].s.nBad == 3 && r[10].gate == 2.0 && r[10].its[1] == 6, "size %zu", r.size());
    }
    {   // the stop flag goes up during a trial: the trial's decision is taken, the iteration counts, nothing follows
        WScript w = plain(); w.it[0][1][0].abort = true;
        std::vector<WSnap> r = check_window("abort during an accepted trial", w);
        CHECK(r.size() == 2 && !r[1].s.rejected && r[1].gate == 2.0 && r[1].its[0] == 2 && r[1].its[1] == 0 && r[1].chi[1] == 0.0, "size %zu", r.size());
        w = plain(); w.it[1][3] = std::vector<Trial>(10, worse); w.it[1][3][1].abort = true;
        r = check_window("abort during a rejected trial", w);
        CHECK(r.size() == 10 && r[8].s.again && r[9].s.rejected && !r[9].s.again && r[9].s.qmax == 2 && r[9].gate == 2.0 && r[9].its[1] == 4 && r[9].rejects == 2 && same_bits(r[9].chi[1], r[7].chi[1]), "size %zu", r.size());
    }
    {   // rejections in the last iteration of the second optimize(): accepted in the end, and rejected to the end (qmax == 10)
        WScript w = plain(); w.it[1][9] = {worse, worse, good, good, good, good, good, good, good, good};
        std::vector<WSnap> r = check_window("late reject", w);
        CHECK(r.size() == 17 && r[15].s.again && !r[16].s.rejected && r[16].gate == 2.0 && r[16].its[1] == 10 && r[16].rejects == 2, "size %zu", r.size());
        w = plain(); w.it[1][9] = std::vector<Trial>(10, worse);
        r = check_window("late reject to qmax", w);
        CHECK(r.size() == 24 && r[23].s.rejected && r[23].s.qmax == 10 && r[23].gate == 2.0 && r[23].its[1] == 10 && r[23].rejects == 10 && same_bits(r[23].chi[1], r[13].chi[1]), "size %zu", r.size());
    }
    {   // 2 000 seeded random windows of the same mix as below, one trial in 200 with the stop flag going up
        std::mt19937_64 wr(20260511u);
        auto wuni = [&](double a, double b) { return a + (b - a) * (double)(wr() >> 11) * (1.0 / 9007199254740992.0); };
        for (int s = 0; s < 2000 && failures <= 20; s++) {
            WScript w;
            for (int ph = 0; ph < 2; ph++) {
                w.chi0[ph] = pow(10.0, wuni(-2, 4)); w.max_diag[ph] = pow(10.0, wuni(-3, 6));
                for (int it = 0; it < (ph == 0 ? 5 : 10); it++) {
                    std::vector<Trial> t;
                    for (int q = 0; q < 10; q++) {
                        const double u = wuni(0, 1), scale = w.chi0[ph] * wuni(-0.2, 1.0);
                        // (a failed factorisation leaves a zero step: computeScale() is 0, which is what the kernels hand lba_decide then)
                        Trial x = u < 0.04 ? Trial{false, wuni(0.1, 1.0), 0.0, true} : u < 0.05 ? Trial{true, inf, scale, false} : u < 0.06 ? Trial{true, nan, scale, false} : u < 0.08 ? Trial{true, 1.0, scale, true}
                                : u < 0.30 ? Trial{true, wuni(0.9995, 1.0), scale, true} : u < 0.55 ? Trial{true, wuni(1.0, 1.5), scale, true} : Trial{true, wuni(0.2, 1.0), scale, true};
                        x.abort = wuni(0, 1) < 0.005;
                        t.push_back(x);
                    }
                    w.it[ph].push_back(t);
                }
            }
            check_window("random window", w);
        }
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
    printf("lba_ctl: %ld window trials compared\n", n_window_trials);
    printf("lm_core ok\n");
    return 0;
}
