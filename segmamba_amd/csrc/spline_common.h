// The cubic B-spline prefilter's constants, shared by resample.hip (the line padded by 12 edge copies) and augment.hip (the bare line).
#pragma once

namespace segm {

constexpr double kPole = -0.26794919243112270647;                      // sqrt(3) - 2
constexpr double kGain = (1.0 - kPole) * (1.0 - 1.0 / kPole);          // 6
constexpr double kFir0 = kGain * (-kPole / (1.0 - kPole * kPole));     // sqrt(3)
constexpr int kFirTaps = 32;            // the closed-form FIR h_k = kFir0 * z^|k| is cut at |k| = 32 (z^33 = 1e-19)
constexpr int kInitTerms = 40;          // scipy's causal start value, cut where the pole's power no longer counts (z^40 = 1e-23)
constexpr int kLineBatch = 8;           // loads of a line go eight at a time ahead of the recursion that consumes them

}  // namespace segm
