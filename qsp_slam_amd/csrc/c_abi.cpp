// c_abi.cpp -- library-wide C-ABI entry points (version, error text, device count) and the object map-point gate.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "object_gate.hpp"

namespace qsp {
std::string& last_error_ref() {
    static thread_local std::string e;
    return e;
}
// csrc/essential_graph.hpp (compiled with the solver's kernels in ba_solver.hip)
int essential_graph_optimize(int device, int32_t n_kf, const double* sim3_in, const uint8_t* fixed, int32_t n_edge, const int32_t* edge_v0,
                             const int32_t* edge_v1, const double* meas, int32_t fix_scale, int32_t n_iter, double lambda_init,
                             int32_t n_pt, const double* pt_in, const int32_t* pt_ref, double* sim3_out, double* pt_out,
                             qsp_essential_trace* trace);
int essential_graph_stages(int device, int32_t n_kf, const double* sim3_in, const uint8_t* fixed, int32_t n_edge, const int32_t* edge_v0,
                           const int32_t* edge_v1, const double* meas, int32_t fix_scale, double lambda, double* E, double* chi, double* J,
                           double* H, double* b, double* x, double* sim3_trial, double* info);
// csrc/sim3_ransac.hpp (compiled there as well)
int sim3_ransac_batch(int device, int32_t n_cand, const int32_t* match_off, const int32_t* n_its, const int32_t* trip_off,
                      const int32_t* triples, const float* K1, const float* K2, const float* X1c, const float* X2c, const float* sigma2_1,
                      const float* sigma2_2, int32_t min_inliers, int32_t fix_scale, int32_t* first_it, float* R12, float* t12, float* s12,
                      uint8_t* inlier, int32_t* n_inliers, int32_t* hyp_inliers);
// csrc/search_sim3.hpp (compiled there as well)
int search_by_sim3_batch(int device, const qsp_search_sim3_in* in, qsp_search_sim3_out* out);
// csrc/search_bow.hpp (compiled there as well)
int search_by_bow_batch(int device, const qsp_search_bow_in* in, qsp_search_bow_out* out);
}  // namespace qsp

extern "C" const char* qsp_last_error(void) { return qsp::last_error_ref().c_str(); }
extern "C" int qsp_version(void) { return 1; }
extern "C" int qsp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" int qsp_essential_graph_optimize(int device, int32_t n_kf, const double* sim3_in, const uint8_t* fixed, int32_t n_edge,
                                            const int32_t* edge_v0, const int32_t* edge_v1, const double* meas, int32_t fix_scale,
                                            int32_t n_iter, double lambda_init, int32_t n_pt, const double* pt_in,
                                            const int32_t* pt_ref, double* sim3_out, double* pt_out, qsp_essential_trace* trace) {
    return qsp::essential_graph_optimize(device, n_kf, sim3_in, fixed, n_edge, edge_v0, edge_v1, meas, fix_scale, n_iter, lambda_init,
                                         n_pt, pt_in, pt_ref, sim3_out, pt_out, trace);
}
extern "C" int qsp_essential_graph_stages(int device, int32_t n_kf, const double* sim3_in, const uint8_t* fixed, int32_t n_edge,
                                          const int32_t* edge_v0, const int32_t* edge_v1, const double* meas, int32_t fix_scale,
                                          double lambda, double* E, double* chi, double* J, double* H, double* b, double* x,
                                          double* sim3_trial, double* info) {
    return qsp::essential_graph_stages(device, n_kf, sim3_in, fixed, n_edge, edge_v0, edge_v1, meas, fix_scale, lambda, E, chi, J, H, b, x,
                                       sim3_trial, info);
}
extern "C" int qsp_sim3_ransac_batch(int device, int32_t n_cand, const int32_t* match_off, const int32_t* n_its, const int32_t* trip_off,
                                     const int32_t* triples, const float* K1, const float* K2, const float* X1c, const float* X2c,
                                     const float* sigma2_1, const float* sigma2_2, int32_t min_inliers, int32_t fix_scale,
                                     int32_t* first_it, float* R12, float* t12, float* s12, uint8_t* inlier, int32_t* n_inliers,
                                     int32_t* hyp_inliers) {
    return qsp::sim3_ransac_batch(device, n_cand, match_off, n_its, trip_off, triples, K1, K2, X1c, X2c, sigma2_1, sigma2_2, min_inliers,
                                  fix_scale, first_it, R12, t12, s12, inlier, n_inliers, hyp_inliers);
}
extern "C" int qsp_search_by_sim3_batch(int device, const qsp_search_sim3_in* in, qsp_search_sim3_out* out) {
    return qsp::search_by_sim3_batch(device, in, out);
}
extern "C" int qsp_search_by_bow_batch(int device, const qsp_search_bow_in* in, qsp_search_bow_out* out) {
    return qsp::search_by_bow_batch(device, in, out);
}
extern "C" int qsp_object_gates(int device, const qsp_object_gate_in* in, qsp_object_gate_out* out) {
    return qsp::object_gates(device, in, out);
}
