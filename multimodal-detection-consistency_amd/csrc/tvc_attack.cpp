// C-ABI of the FSTA / SMA attack kernels (attack.hip): tvc_attack_feature_grad / tvc_attack_step.  Its own translation unit:
// nothing here is called from tvc_abi.cpp.  Neither call owns a workspace or reads the handle beyond its error string.
#include "handle.hpp"

int tvc_attack_feature_grad(tvc_handle* h, const float* f_dev, const float* t_dev, const float* g_dev, int32_t B, int32_t D,
                            float a_tgt, float a_txt, int32_t metric, float w_out, float w_div, float* grad_dev,
                            float* loss_rows_dev, void* stream) {
    if (!h) return TVC_E_INVALID;
    if (B < 0 || D < 0) return fail(h, TVC_E_INVALID, "tvc_attack_feature_grad: B and D must not be negative");
    if (metric != TVC_ATTACK_METRIC_COSINE && metric != TVC_ATTACK_METRIC_EUCLIDEAN)
        return fail(h, TVC_E_INVALID, "tvc_attack_feature_grad: metric must be TVC_ATTACK_METRIC_COSINE or TVC_ATTACK_METRIC_EUCLIDEAN");
    if (B == 0 || D == 0) return TVC_OK;
    if (!f_dev || !t_dev || !g_dev || !grad_dev || !loss_rows_dev)
        return fail(h, TVC_E_INVALID, "tvc_attack_feature_grad: f, t, g, grad and loss_rows must not be NULL");
    if (grad_dev == f_dev || grad_dev == t_dev || grad_dev == g_dev)
        return fail(h, TVC_E_INVALID, "tvc_attack_feature_grad: grad must not alias an input (every row reads all of f)");
    HIP_TRY(launch_attack_feature_grad(f_dev, t_dev, g_dev, B, D, a_tgt, a_txt, metric == TVC_ATTACK_METRIC_EUCLIDEAN, w_out, w_div,
                                       grad_dev, loss_rows_dev, (hipStream_t)stream));
    return TVC_OK;
}

int tvc_attack_step(tvc_handle* h, float* adv_dev, const float* clean_dev, const float* grad_dev, float* mom_dev, int32_t B,
                    int64_t n, float eps, float lr, float mu, float clip, float p, float clip_min, float clip_max, int32_t norm,
                    void* stream) {
    if (!h) return TVC_E_INVALID;
    if (B < 0 || n < 0) return fail(h, TVC_E_INVALID, "tvc_attack_step: B and n must not be negative");
    if (norm != TVC_ATTACK_NORM_INF && norm != TVC_ATTACK_NORM_L2)
        return fail(h, TVC_E_INVALID, "tvc_attack_step: norm must be TVC_ATTACK_NORM_INF or TVC_ATTACK_NORM_L2");
    if (!(eps >= 0.f)) return fail(h, TVC_E_INVALID, "tvc_attack_step: eps must be a number >= 0");
    if (!(clip_min <= clip_max)) return fail(h, TVC_E_INVALID, "tvc_attack_step: need clip_min <= clip_max");
    if (B == 0 || n == 0) return TVC_OK;
    if (!adv_dev || !clean_dev || !grad_dev || !mom_dev)
        return fail(h, TVC_E_INVALID, "tvc_attack_step: adv, clean, grad and mom must not be NULL");
    HIP_TRY(launch_attack_step(adv_dev, clean_dev, grad_dev, mom_dev, B, n, eps, lr, mu, clip, p, clip_min, clip_max,
                               norm == TVC_ATTACK_NORM_L2, (hipStream_t)stream));
    return TVC_OK;
}
