/* C++11 mirror of the member surface FullSystem uses on the photometric alignment path, over the C ABI of dmvio_hip.h.
 *
 * The reference has no plugin / FFI interface on this path — its boundary is the C++ member surface of CoarseTracker and FrameHessian
 * (SURVEY.md section 8b).  These classes keep the reference's names, argument meaning and error behaviour (bool results, NaN residuals, no
 * exceptions) with plain-old-data in place of Eigen / Sophus types, so that an adapter inside the reference is a field-by-field copy:
 *
 *   dmvio_hip::FrameStore::makeImages(slot, color)          <- FrameHessian::makeImages(float* color, CalibHessian*)   HessianBlocks.cpp:128-191
 *   dmvio_hip::CoarseTracker::makeK(fx, fy, cx, cy)          <- CoarseTracker::makeK(CalibHessian*)                      CoarseTracker.cpp:105-134
 *   dmvio_hip::CoarseTracker::setCoarseTrackingRef(...)      <- CoarseTracker::setCoarseTrackingRef(frameHessians)       CoarseTracker.cpp:524-538
 *   dmvio_hip::CoarseTracker::trackNewestCoarse(...)         <- CoarseTracker::trackNewestCoarse(newFH, lastToNew_out, aff_g2l_out, coarsestLvl,
 *                                                               minResForAbort)                                          CoarseTracker.cpp:539-770
 *   members lastResiduals, lastFlowIndicators, refFrameID    <- CoarseTracker.h:83-91
 *
 * Header-only; link with -ldmvio_hip.  Not thread-safe per object, like the reference's tracker (one tracker per thread). */
#ifndef DMVIO_HIP_HPP
#define DMVIO_HIP_HPP
#include <algorithm>
#include <cmath>
#include <functional>
#include <string>
#include <vector>
#include "dmvio_hip.h"

namespace dmvio_hip {

/* Sophus::SE3d as [translation | unit quaternion x y z w] (the pose7 of the C ABI) */
struct SE3 {
  double t[3];
  double q[4];
  SE3() { t[0] = t[1] = t[2] = 0; q[0] = q[1] = q[2] = 0; q[3] = 1; }
  void toPose7(double p[7]) const { for (int i = 0; i < 3; i++) p[i] = t[i]; for (int i = 0; i < 4; i++) p[3 + i] = q[i]; }
  void fromPose7(const double p[7]) { for (int i = 0; i < 3; i++) t[i] = p[i]; for (int i = 0; i < 4; i++) q[i] = p[3 + i]; }
};
/* dso::AffLight (util/NumType.h:166-192) */
struct AffLight {
  double a, b;
  AffLight() : a(0), b(0) {}
  AffLight(double a_, double b_) : a(a_), b(b_) {}
};

inline std::string lastError() { const char* e = dmvio_hip_last_error(); return e ? e : ""; }

/* The resident image pyramids: one slot per FrameHessian that is alive (its dIp pyramid in the reference). */
class FrameStore {
 public:
  FrameStore(int device, int w, int h, int n_slots) : ctx_(dmvio_hip_create(device, w, h, n_slots)), w_(w), h_(h) {}
  ~FrameStore() { if (ctx_) dmvio_hip_destroy(ctx_); }
  FrameStore(const FrameStore&) = delete;
  FrameStore& operator=(const FrameStore&) = delete;
  bool valid() const { return ctx_ != nullptr; }
  int pyrLevelsUsed() const { return ctx_ ? dmvio_hip_pyr_levels(ctx_) : 0; }
  int w() const { return w_; }
  int h() const { return h_; }
  /* FrameHessian::makeImages: irradiance image (w*h floats) -> pyramid of the slot */
  bool makeImages(int slot, const float* color) { return ctx_ && dmvio_hip_frame_upload(ctx_, slot, color) == 0; }
  /* the same for images that stay resident in device memory: level 0 is the image itself */
  bool makeImagesInPlace(int n, const int* slots, const float* device_images, size_t stride_bytes) {
    return ctx_ && dmvio_hip_frames_attach_device_batch(ctx_, n, slots, device_images, stride_bytes) == 0;
  }
  /* FrameHessian::absSquaredGrad[0..2] of a resident frame (HessianBlocks.cpp:169-189), what PixelSelector::makeMaps reads; B = CalibHessian::B (256 floats) for the
   * getBGradOnly weights of setting_gammaWeightsPixelSelect == 1, or NULL.  out[l] must hold (w >> l) * (h >> l) floats. */
  bool absSquaredGrad(int slot, const float* B, float* const out[3]) { return ctx_ && dmvio_hip_frame_abs_squared_grad(ctx_, slot, 3, B, out) == 0; }
  dmvio_hip_ctx* handle() const { return ctx_; }

 private:
  dmvio_hip_ctx* ctx_;
  int w_, h_;
};

/* One active point of the reference keyframe as setCoarseTrackingRef reads it (CoarseTracker.cpp:144-161): centerProjectedTo of the
 * residual that targets lastRef, and efPoint->HdiF. */
struct RefPoint { float u, v, idepth, HdiF; };

class CoarseTracker {
 public:
  explicit CoarseTracker(FrameStore& frames) : refFrameID(-1), frames_(frames), trk_(frames.valid() ? dmvio_hip_tracker_create(frames.handle()) : nullptr), refSlot_(-1) {
    for (int i = 0; i < 5; i++) lastResiduals[i] = NAN;
    for (int i = 0; i < 3; i++) lastFlowIndicators[i] = 1000;
  }
  ~CoarseTracker() { if (trk_) dmvio_hip_tracker_destroy(trk_); }
  CoarseTracker(const CoarseTracker&) = delete;
  CoarseTracker& operator=(const CoarseTracker&) = delete;

  bool makeK(float fx, float fy, float cx, float cy) {
    const float K[4] = {fx, fy, cx, cy};
    return trk_ && dmvio_hip_tracker_make_k(trk_, K) == 0;
  }
  /* lastRef = the newest keyframe (its slot, frameID, ab_exposure, aff_g2l); points = the active points with an IN residual into it */
  bool setCoarseTrackingRef(int refSlot, int frameID, float ab_exposure, const AffLight& aff_g2l, const std::vector<RefPoint>& points) {
    if (!trk_) return false;
    const size_t n = points.size();
    std::vector<float> u(n), v(n), id(n), hd(n);
    for (size_t i = 0; i < n; i++) { u[i] = points[i].u; v[i] = points[i].v; id[i] = points[i].idepth; hd[i] = points[i].HdiF; }
    if (dmvio_hip_tracker_set_ref(trk_, refSlot, ab_exposure, aff_g2l.a, aff_g2l.b, (int)n, u.data(), v.data(), id.data(), hd.data()) != 0) return false;
    refSlot_ = refSlot; refFrameID = frameID; lastRef_aff_g2l = aff_g2l;
    return true;
  }
  /* the same with the points read from a resident window optimiser (dmvio_hip_tracker_set_ref_from_ba): the residuals into its newest keyframe that are active and IN,
   * in graph order; nothing is gathered on the host.  nSelected (may be NULL): how many there were */
  bool setCoarseTrackingRefFromBA(dmvio_hip_ba* ba, int refSlot, int frameID, float ab_exposure, const AffLight& aff_g2l, int* nSelected = nullptr) {
    if (!trk_ || dmvio_hip_tracker_set_ref_from_ba(trk_, ba, refSlot, ab_exposure, aff_g2l.a, aff_g2l.b, nSelected) != 0) return false;
    refSlot_ = refSlot; refFrameID = frameID; lastRef_aff_g2l = aff_g2l;
    return true;
  }
  /* idepth[lvl] / weightSums[lvl] of the current template (w_lvl * h_lvl floats each): the arrays debugPlotIDepthMap / debugPlotIDepthMapFloat read (CoarseTracker.cpp:772-880) */
  bool idepthMap(int lvl, std::vector<float>& idepth, std::vector<float>& weightSums) const {
    if (!trk_ || lvl < 0 || lvl >= frames_.pyrLevelsUsed()) return false;
    const size_t n = (size_t)(frames_.w() >> lvl) * (frames_.h() >> lvl);
    idepth.resize(n); weightSums.resize(n);
    return dmvio_hip_tracker_get_idepth_map(trk_, lvl, idepth.data(), weightSums.data()) == 0;
  }
  /* Returns trackingGood; lastToNew_out / aff_g2l_out are written only when every level finished (CoarseTracker.cpp:731-760); a device or
   * argument error reads as "tracking failed" (the adapter sets isLost), lastError() tells why. */
  bool trackNewestCoarse(int newSlot, float new_ab_exposure, SE3& lastToNew_out, AffLight& aff_g2l_out, int coarsestLvl, const double minResForAbort[5]) {
    if (!trk_) return false;
    double pose7[7], aff[2] = {aff_g2l_out.a, aff_g2l_out.b};
    lastToNew_out.toPose7(pose7);
    int good = 0;
    if (dmvio_hip_tracker_track(trk_, newSlot, new_ab_exposure, pose7, aff, coarsestLvl, minResForAbort, lastResiduals, lastFlowIndicators, lastH, lastb, &good) != 0) return false;
    lastToNew_out.fromPose7(pose7);
    aff_g2l_out = AffLight(aff[0], aff[1]);
    return good != 0;
  }
  /* The reference's default branch (setting_useIMU, CoarseTracker.cpp:612-637): every LM step is computed by the caller.  The three
   * members mirror what the tracker calls on dmvio::IMUIntegration (IMUIntegration.hpp:106-112):
   *   computeCoarseUpdate(H, b, extrapFac, lambda, incA, incB, incNorm) -> refToNew_new      H: 8x8 row-major, scaled, [trans rot a b]
   *   acceptCoarseUpdate()
   *   addVisualToCoarseGraph(H, b, trackingGood)
   * An empty computeCoarseUpdate runs the visual-only step (what the reference does while !isCoarseInitialized()). */
  struct CoarseIMUHooks {
    std::function<SE3(const double* H, const double* b, float extrapFac, float lambda, const SE3& refToNew_current, double& incA, double& incB, double& incNorm)>
        computeCoarseUpdate;
    std::function<void()> acceptCoarseUpdate;
    std::function<void(const double* H, const double* b, bool trackingGood)> addVisualToCoarseGraph;
  };
  bool trackNewestCoarse(int newSlot, float new_ab_exposure, SE3& lastToNew_out, AffLight& aff_g2l_out, int coarsestLvl, const double minResForAbort[5],
                         const CoarseIMUHooks& imu) {
    if (!trk_) return false;
    dmvio_hip_coarse_callbacks cb;
    cb.user = const_cast<CoarseIMUHooks*>(&imu);
    cb.update = imu.computeCoarseUpdate ? &CoarseTracker::updateThunk : nullptr;
    cb.accept = imu.acceptCoarseUpdate ? &CoarseTracker::acceptThunk : nullptr;
    cb.visual = imu.addVisualToCoarseGraph ? &CoarseTracker::visualThunk : nullptr;
    double pose7[7], aff[2] = {aff_g2l_out.a, aff_g2l_out.b};
    lastToNew_out.toPose7(pose7);
    int good = 0;
    if (dmvio_hip_tracker_track_vio(trk_, newSlot, new_ab_exposure, pose7, aff, coarsestLvl, minResForAbort, &cb, lastResiduals, lastFlowIndicators, lastH, lastb, &good,
                                    &lastEvaluations) != 0)
      return false;
    lastToNew_out.fromPose7(pose7);
    aff_g2l_out = AffLight(aff[0], aff[1]);
    return good != 0;
  }
  int lastEvaluations = 0;   /* calcRes + calcGSSSE passes of the last hand-off track */
  int pc_n(int lvl) const { return trk_ ? dmvio_hip_tracker_pc_n(trk_, lvl) : 0; }
  /* the C handle, for calls that take several trackers (TrackMulti::track); stays owned by this object */
  dmvio_hip_tracker* handle() const { return trk_; }

  /* CoarseTracker.h:83-91 */
  double lastResiduals[5];
  double lastFlowIndicators[3];
  AffLight lastRef_aff_g2l;
  int refFrameID;
  /* the scaled 8x8 system at the accepted state of the last level — what IMUIntegration::addVisualToCoarseGraph receives (CoarseTracker.cpp:766) */
  double lastH[64], lastb[8];

 private:
  static int updateThunk(void* user, const double H[64], const double b[8], float extrapFac, float lambda, const double pose7_cur[7], const double*, double pose7_new[7],
                         double* incA, double* incB, double* incNorm) {
    const CoarseIMUHooks* h = static_cast<const CoarseIMUHooks*>(user);
    SE3 cur; cur.fromPose7(pose7_cur);
    const SE3 nxt = h->computeCoarseUpdate(H, b, extrapFac, lambda, cur, *incA, *incB, *incNorm);
    nxt.toPose7(pose7_new);
    return 0;
  }
  static void acceptThunk(void* user) { static_cast<const CoarseIMUHooks*>(user)->acceptCoarseUpdate(); }
  static void visualThunk(void* user, const double H[64], const double b[8], int good) { static_cast<const CoarseIMUHooks*>(user)->addVisualToCoarseGraph(H, b, good != 0); }
  FrameStore& frames_;
  dmvio_hip_tracker* trk_;
  int refSlot_;
};

/* ---- mapping side: the window FullSystem::optimize works on -------------------------------------------------------------------------
 *   KeyFrame      <- FrameHessian (slot of its pyramid, worldToCam_evalPT, aff_g2l, ab_exposure, frameID)       HessianBlocks.h:113-307
 *   ActivePoint   <- PointHessian (host frame index, u, v, idepth, color[8], weights[8], hasDepthPrior) with the targets of its residuals
 *                                                                                                                HessianBlocks.h:413-508
 *   WindowOptimizer::optimize(mnumOptIts) <- float FullSystem::optimize(int)                                     FullSystemOptimize.cpp:417-647 */
struct KeyFrame {
  int slot;
  SE3 worldToCam_evalPT;
  AffLight aff_g2l;
  float ab_exposure;
  int frameID;
};
struct ActivePoint {
  int host;
  float u, v, idepth;
  float color[8], weights[8];
  bool hasDepthPrior;
  std::vector<int> targets;   /* frame indices of its PointFrameResiduals */
};

/* The window's point / residual graph kept resident across keyframes: EnergyFunctional's own mutators over a host-side mirror (dmvio_hip_graph_*, include/dmvio_hip.h
 * "window graph"; EnergyFunctional.cpp:435-518, 641-646, 766-782).  Elements are addressed as the reference addresses its objects: a keyframe by EFFrame::idx, a point by
 * (host keyframe, EFPoint::idxInPoints), a residual by (point, EFResidual::idxInAll); insert* return the index the reference assigns in the same call, -1 on error. */
class WindowGraph {
 public:
  WindowGraph() : g_(dmvio_hip_graph_create()) {}
  ~WindowGraph() { if (g_) dmvio_hip_graph_destroy(g_); }
  WindowGraph(const WindowGraph&) = delete;
  WindowGraph& operator=(const WindowGraph&) = delete;
  bool valid() const { return g_ != nullptr; }
  int insertFrame() { return g_ ? dmvio_hip_graph_insert_frame(g_) : -1; }
  bool marginalizeFrame(int idx) { return g_ && dmvio_hip_graph_remove_frame(g_, idx) == 0; }
  int insertPoint(const ActivePoint& p) { return g_ ? dmvio_hip_graph_insert_point(g_, p.host, p.u, p.v, p.idepth, p.color, p.weights, p.hasDepthPrior ? 1 : 0) : -1; }
  bool removePoint(int host, int idxInPoints) { return g_ && dmvio_hip_graph_remove_point(g_, host, idxInPoints) == 0; }
  int insertResidual(int host, int idxInPoints, int target) { return g_ ? dmvio_hip_graph_insert_residual(g_, host, idxInPoints, target) : -1; }
  bool dropResidual(int host, int idxInPoints, int idxInAll) { return g_ && dmvio_hip_graph_drop_residual(g_, host, idxInPoints, idxInAll) == 0; }
  bool setIdepth(int host, int idxInPoints, float idepth) { return g_ && dmvio_hip_graph_set_idepth(g_, host, idxInPoints, idepth) == 0; }
  bool setIdepths(const std::vector<float>& idepth) { return g_ && dmvio_hip_graph_set_idepths(g_, (int)idepth.size(), idepth.data()) == 0; }   /* makeIDX order */
  /* EFResidual::fixLinearizationF's result of one residual (isLinearized = true with its 74-float RawResidualJacobian and res_toZeroF), or isLinearized = false again
   * (J74 == nullptr): the record follows the residual through dropResidual / removePoint and WindowOptimizer::setGraphFrom hands it over */
  bool setResidualLinearized(int host, int idxInPoints, int idxInAll, const float* J74, const float* resToZeroF8) {
    return g_ && dmvio_hip_graph_set_residual_linearized(g_, host, idxInPoints, idxInAll, J74, resToZeroF8) == 0;
  }
  int nLinearized() const { return g_ ? dmvio_hip_graph_linearized_count(g_) : -1; }
  int nFrames() const { int F = 0; return g_ && dmvio_hip_graph_counts(g_, &F, nullptr, nullptr) == 0 ? F : -1; }
  int nPoints() const { int N = 0; return g_ && dmvio_hip_graph_counts(g_, nullptr, &N, nullptr) == 0 ? N : -1; }
  int nResiduals() const { int R = 0; return g_ && dmvio_hip_graph_counts(g_, nullptr, nullptr, &R) == 0 ? R : -1; }
  dmvio_hip_graph* handle() const { return g_; }

 private:
  dmvio_hip_graph* g_;
};

class WindowOptimizer {
 public:
  explicit WindowOptimizer(FrameStore& frames) : lastEnergy(NAN), lastIterations(0), ba_(frames.valid() ? dmvio_hip_ba_create(frames.handle()) : nullptr), F_(0), N_(0) {}
  ~WindowOptimizer() { if (ba_) dmvio_hip_ba_destroy(ba_); }
  WindowOptimizer(const WindowOptimizer&) = delete;
  WindowOptimizer& operator=(const WindowOptimizer&) = delete;

  /* frameHessians in window order (newest last) + Hcalib: EnergyFunctional::insertFrame / setAdjointsF / FullSystem::setPrecalcValues */
  bool setWindow(const std::vector<KeyFrame>& frameHessians, double fx, double fy, double cx, double cy) {
    if (!ba_) return false;
    const int F = (int)frameHessians.size();
    std::vector<int> slots(F), ids(F);
    std::vector<double> poses(7 * (size_t)F), aff(2 * (size_t)F);
    std::vector<float> expo(F);
    for (int f = 0; f < F; f++) {
      slots[f] = frameHessians[f].slot; ids[f] = frameHessians[f].frameID; expo[f] = frameHessians[f].ab_exposure;
      frameHessians[f].worldToCam_evalPT.toPose7(&poses[7 * (size_t)f]);
      aff[2 * (size_t)f] = frameHessians[f].aff_g2l.a; aff[2 * (size_t)f + 1] = frameHessians[f].aff_g2l.b;
    }
    const double K[4] = {fx, fy, cx, cy};
    if (dmvio_hip_ba_set_window(ba_, F, slots.data(), poses.data(), aff.data(), expo.data(), ids.data(), K) != 0) return false;
    F_ = F;
    return true;
  }
  /* all active points in allPoints order with their residuals: EnergyFunctional::makeIDX */
  bool setPoints(const std::vector<ActivePoint>& points) {
    if (!ba_) return false;
    const size_t N = points.size();
    std::vector<int> host(N), rp, rt;
    std::vector<float> u(N), v(N), id(N), col(8 * N), wts(8 * N);
    std::vector<unsigned char> prior(N);
    for (size_t i = 0; i < N; i++) {
      host[i] = points[i].host; u[i] = points[i].u; v[i] = points[i].v; id[i] = points[i].idepth; prior[i] = points[i].hasDepthPrior ? 1 : 0;
      for (int k = 0; k < 8; k++) { col[8 * i + k] = points[i].color[k]; wts[8 * i + k] = points[i].weights[k]; }
      for (size_t r = 0; r < points[i].targets.size(); r++) { rp.push_back((int)i); rt.push_back(points[i].targets[r]); }
    }
    if (dmvio_hip_ba_set_graph(ba_, (int)N, host.data(), u.data(), v.data(), id.data(), col.data(), wts.data(), prior.data(), (int)rp.size(), rp.data(), rt.data()) != 0) return false;
    N_ = (int)N;
    return true;
  }
  /* the same from a resident WindowGraph (no flat arrays are formed by the caller); after optimize(): graph.setIdepths(<idepths()>) */
  bool setPoints(const WindowGraph& graph) {
    if (!ba_ || !graph.valid() || dmvio_hip_ba_set_graph_from(ba_, graph.handle()) != 0) return false;
    N_ = graph.nPoints();
    return true;
  }
  /* returns sqrt(E / (patternNum * resInA)) like the reference; a negative value on a device / argument error (the adapter sets isLost) */
  float optimize(int mnumOptIts) {
    if (!ba_) return -1.0f;
    float rmse = -1.0f;
    if (dmvio_hip_ba_optimize(ba_, mnumOptIts, &rmse, &lastEnergy, &lastIterations, energyTrace) != 0) return -1.0f;
    return rmse;
  }
  /* FullSystem::optimize on the reference's default branch (setting_useGTSAMIntegration): the members of dmvio::BAGTSAMIntegration the loop calls as hooks
   * (computeBAUpdate / getBAEnergy / updateBAValues / updateDynamicWeight / canBreak / acceptBAUpdate / postOptimization, include/dmvio_hip.h), the options what the
   * reference reads beside them (shell->trackingWasGood, updateDynamicWeightDuringOptimization, setting_minOptIterations, ef->resInA, HMForGTSAM / bMForGTSAM) */
  float optimize(int mnumOptIts, const dmvio_hip_ba_callbacks& hooks, const dmvio_hip_ba_vio_options& options) {
    if (!ba_) return -1.0f;
    float rmse = -1.0f;
    if (dmvio_hip_ba_optimize_vio(ba_, mnumOptIts, &hooks, &options, &rmse, &lastEnergy, &lastIterations, energyTrace) != 0) return -1.0f;
    return rmse;
  }
  /* one window over several GPUs: this optimizer holds all keyframes and the rank's share of the points; with a communicator set, optimize() is collective (every rank
   * calls it) and runs the all-reduce of the system and the all-gather of the decision records itself, on its own stream (include/dmvio_hip.h, dmvio_hip_ba_set_comm) */
  bool setCommunicator(void* ncclComm, int rank, int world) { return ba_ && dmvio_hip_ba_set_comm(ba_, ncclComm, rank, world) == 0; }
  /* 1 = the reference's single-threaded accumulation order (bit-identical sums); default 4 partial accumulators per bucket = its multi-threaded structure */
  bool setAccumulators(int k) { return ba_ && dmvio_hip_ba_set_accumulators(ba_, k) == 0; }
  bool frameState(int f, SE3& worldToCam, AffLight& aff_g2l) const {
    double p[7], a[2], st[10];
    if (!ba_ || dmvio_hip_ba_get_frame(ba_, f, p, a, st) != 0) return false;
    worldToCam.fromPose7(p); aff_g2l = AffLight(a[0], a[1]);
    return true;
  }
  bool idepths(std::vector<float>& idepth) const {
    idepth.resize(N_);
    return ba_ && dmvio_hip_ba_get_points(ba_, idepth.data(), nullptr) == 0;
  }
  /* EFResidual::fixLinearizationF for the active residuals with mask != 0 on the resident graph (outside a marginalisation): from then on they ride in every system through
   * accumulateLF_MT / addPoint<1> and in E_L through calcLEnergyPt; needs keepJacobians(true) before the optimize that precedes it.  Returns the number of linearised
   * residuals of the graph, -1 on error. */
  int fixLinearization(const std::vector<unsigned char>& residualMask) {
    int n = -1;
    if (!ba_ || dmvio_hip_ba_fix_linearization(ba_, (int)residualMask.size(), residualMask.data(), &n) != 0) return -1;
    return n;
  }
  /* residuals that ARRIVE linearised with a flat graph (right after setGraph): flags, 74-float Jacobians and res_toZeroF per residual, graph order; and what the window holds,
   * to be handed to the next one.  Returns the number of linearised residuals, -1 on error. */
  int setLinearizedResiduals(const std::vector<unsigned char>& isLinearized, const std::vector<float>& J74, const std::vector<float>& resToZeroF8) {
    int n = -1;
    const size_t R = isLinearized.size();
    if (!ba_ || J74.size() != 74 * R || resToZeroF8.size() != 8 * R) return -1;
    if (dmvio_hip_ba_set_linearized_residuals(ba_, (int)R, isLinearized.data(), J74.data(), resToZeroF8.data(), &n) != 0) return -1;
    return n;
  }
  bool linearizedResiduals(int R, std::vector<unsigned char>& isLinearized, std::vector<float>& J74, std::vector<float>& resToZeroF8) const {
    isLinearized.resize(R); J74.resize(74 * (size_t)R); resToZeroF8.resize(8 * (size_t)R);
    return ba_ && dmvio_hip_ba_get_linearized_residuals(ba_, R, isLinearized.data(), J74.data(), resToZeroF8.data()) == 0;
  }
  bool keepJacobians(bool on) { return ba_ && dmvio_hip_ba_keep_jacobians(ba_, on ? 1 : 0) == 0; }
  dmvio_hip_ba* handle() const { return ba_; }
  double lastEnergy;           /* E_A + E_L + E_M after the last optimize */
  int lastIterations;
  double energyTrace[64 * 4];  /* per iteration: E_A, E_L, E_M, accepted (row 0: before the first step) */

 private:
  dmvio_hip_ba* ba_;
  int F_, N_;
  friend class WindowBatch;
};

/* FullSystem::optimize for several windows per call (dmvio_hip_ba_optimize_batch): the whole Gauss-Newton loop — the 68x68 solve, the frame step and the accept test included —
 * runs on the device for all of them, two host waits per call.  Each WindowOptimizer is set up as for its own optimize(); its results are read with its own getters afterwards. */
class WindowBatch {
 public:
  WindowBatch(dmvio_hip_ctx* ctx, int maxWindows) : b_(dmvio_hip_ba_batch_create(ctx, maxWindows)) {}
  ~WindowBatch() { if (b_) dmvio_hip_ba_batch_destroy(b_); }
  WindowBatch(const WindowBatch&) = delete;
  WindowBatch& operator=(const WindowBatch&) = delete;
  bool valid() const { return b_ != nullptr; }
  /* rmse[i] = sqrt(E / (patternNum * resInA)) of window i like the reference's return value; false on a device / argument error */
  bool optimize(const std::vector<WindowOptimizer*>& windows, int mnumOptIts, std::vector<float>& rmse) {
    if (!b_ || windows.empty()) return false;
    std::vector<dmvio_hip_ba*> hs(windows.size());
    for (size_t i = 0; i < windows.size(); i++) { if (!windows[i] || !windows[i]->ba_) return false; hs[i] = windows[i]->ba_; }
    rmse.assign(windows.size(), -1.0f);
    std::vector<double> energy(windows.size()), trace(windows.size() * 256);
    std::vector<int> its(windows.size());
    if (dmvio_hip_ba_optimize_batch(b_, (int)hs.size(), hs.data(), mnumOptIts, rmse.data(), energy.data(), its.data(), trace.data()) != 0) return false;
    for (size_t i = 0; i < windows.size(); i++) {
      windows[i]->lastEnergy = energy[i]; windows[i]->lastIterations = its[i];
      for (int k = 0; k < 256; k++) windows[i]->energyTrace[k] = trace[i * 256 + k];
    }
    return true;
  }

 private:
  dmvio_hip_ba_batch* b_;
};

/* PixelSelector (FullSystem/PixelSelector2.h) on a resident frame: the reference's surface over dmvio_hip_pixel_selector_*.  randomPattern = the w*h table the
 * reference's constructor fills from rand() after srand(3141592) (PixelSelector2.cpp:45-47); the library does not touch the process's rand() state. */
class PixelSelector {
 public:
  PixelSelector(dmvio_hip_ctx* ctx, const unsigned char* randomPattern) : s_(dmvio_hip_pixel_selector_create(ctx, randomPattern)) {}
  ~PixelSelector() { if (s_) dmvio_hip_pixel_selector_destroy(s_); }
  PixelSelector(const PixelSelector&) = delete;
  PixelSelector& operator=(const PixelSelector&) = delete;
  bool valid() const { return s_ != nullptr; }
  /* makeMaps (PixelSelector2.cpp:158-307) of the frame in `slot`; map_out (w*h floats, 0 / 1 / 2 / 4) may be NULL when only the device-resident list is wanted.
   * B = CalibHessian::B for setting_gammaWeightsPixelSelect == 1, or NULL.  Returns numHaveSub, or <0 on an error (lastError()). */
  int makeMaps(int slot, float* map_out, float density, int recursionsLeft = 1, float thFactor = 1, const float* B = nullptr) {
    int n = 0;
    if (!s_) return -1;
    const int r = dmvio_hip_pixel_selector_make_maps(s_, slot, B, density, recursionsLeft, thFactor, &n, nullptr, map_out);
    return r < 0 ? r : n;
  }
  int currentPotential() const { return s_ ? dmvio_hip_pixel_selector_get_potential(s_) : -1; }
  bool setCurrentPotential(int pot) { return s_ && dmvio_hip_pixel_selector_set_potential(s_, pot) == 0; }
  bool setSettings(const dmvio_hip_pixel_selector_settings& st) { return s_ && dmvio_hip_pixel_selector_set_settings(s_, &st) == 0; }
  /* the selected pixels of the last makeMaps in the order FullSystem::makeNewTraces walks the map */
  bool selection(std::vector<int>& u, std::vector<int>& v, std::vector<int>& type) {
    long long st[4];
    if (!s_ || dmvio_hip_pixel_selector_get_stats(s_, st) != 0) return false;
    u.assign((size_t)st[2], 0); v.assign((size_t)st[2], 0); type.assign((size_t)st[2], 0);
    return dmvio_hip_pixel_selector_get_selection(s_, u.data(), v.data(), type.data()) >= 0;
  }
  /* the point-construction loop of FullSystem::makeNewTraces (FullSystem.cpp:1653-1663) for the last makeMaps: index of the first new point of `points`, or <0 */
  int makeNewTraces(dmvio_hip_immature* points, int host_tag, int host_slot) { return s_ ? dmvio_hip_immature_add_selected(points, host_tag, host_slot, s_) : -1; }
  dmvio_hip_pixel_selector* handle() const { return s_; }

 private:
  dmvio_hip_pixel_selector* s_;
};

/* PixelSelector::makeMaps and the point loop of FullSystem::makeNewTraces for several windows per call (dmvio_hip_pixel_selector_batch): W PixelSelector objects and W
 * immature handles of one context.  Every window ends in the state its single calls leave; the results are read from the records and with the windows' own getters
 * (PixelSelector::selection, currentPotential).  A call is refused as a whole (lastError()) before any window is touched. */
class PixelSelectorBatch {
 public:
  PixelSelectorBatch(dmvio_hip_ctx* ctx, int maxWindows) : b_(dmvio_hip_pixel_selector_batch_create(ctx, maxWindows)) {}
  ~PixelSelectorBatch() { if (b_) dmvio_hip_pixel_selector_batch_destroy(b_); }
  PixelSelectorBatch(const PixelSelectorBatch&) = delete;
  PixelSelectorBatch& operator=(const PixelSelectorBatch&) = delete;
  bool valid() const { return b_ != nullptr; }
  /* makeMaps (PixelSelector2.cpp:158-307) of every window: sel, slot, B_lut256, density, recursions_left, th_factor and map_out_host of each record; n_selected and
   * counts3 are written */
  bool makeMaps(std::vector<dmvio_hip_pixel_selector_window>& windows) {
    return b_ && dmvio_hip_pixel_selector_make_maps_batch(b_, (int)windows.size(), windows.data()) == 0;
  }
  /* the point loop of makeNewTraces (FullSystem.cpp:1653-1663) of every window; `first` of each record is written */
  bool makeNewTraces(std::vector<dmvio_hip_new_traces_window>& windows) {
    return b_ && dmvio_hip_immature_add_selected_batch(b_, (int)windows.size(), windows.data()) == 0;
  }
  dmvio_hip_pixel_selector_batch* handle() const { return b_; }

 private:
  dmvio_hip_pixel_selector_batch* b_;
};

/* CoarseDistanceMap (FullSystem/CoarseTracker.h) at pyramid level 1 over dmvio_hip_distance_map_*: the map FullSystem::activatePointsMT tests its candidates against. */
class DistanceMap {
 public:
  explicit DistanceMap(dmvio_hip_ctx* ctx) : d_(dmvio_hip_distance_map_create(ctx)) {}
  ~DistanceMap() { if (d_) dmvio_hip_distance_map_destroy(d_); }
  DistanceMap(const DistanceMap&) = delete;
  DistanceMap& operator=(const DistanceMap&) = delete;
  bool valid() const { return d_ != nullptr; }
  /* the rows KRKi = K[1] * R * Ki[0], Kt = K[1] * t of every keyframe against the newest (CoarseTracker.cpp:949-951); pose7 = tx ty tz qx qy qz qw */
  static bool tablesFromPoses(const double newWorldToCam7[7], int nHosts, const double* hostCamToWorld7, const double fxfycxcy[4], std::vector<float>& KRKi,
                              std::vector<float>& Kt) {
    KRKi.assign(9 * (size_t)nHosts, 0.f); Kt.assign(3 * (size_t)nHosts, 0.f);
    return dmvio_hip_distance_map_tables_from_poses(newWorldToCam7, nHosts, hostCamToWorld7, fxfycxcy, KRKi.data(), Kt.data()) == 0;
  }
  /* makeDistanceMap (CoarseTracker.cpp:931-967) from the window's active points: host index, u, v, idepth_scaled */
  bool makeDistanceMap(const std::vector<float>& KRKi, const std::vector<float>& Kt, const std::vector<int>& host, const std::vector<float>& u, const std::vector<float>& v,
                       const std::vector<float>& idepthScaled) {
    return d_ && dmvio_hip_distance_map_make(d_, (int)(Kt.size() / 3), KRKi.data(), Kt.data(), (int)host.size(), host.data(), u.data(), v.data(), idepthScaled.data()) == 0;
  }
  bool addIntoDistFinal(int u, int v) { return d_ && dmvio_hip_distance_map_add(d_, u, v) == 0; }
  /* fwdWarpedIDDistFinal, (w>>1)*(h>>1) floats */
  bool get(std::vector<float>& map) {
    if (!d_) return false;
    map.assign((size_t)dmvio_hip_distance_map_size(d_, nullptr, nullptr), 0.f);
    return dmvio_hip_distance_map_get(d_, map.data()) == 0;
  }
  dmvio_hip_distance_map* handle() const { return d_; }

 private:
  dmvio_hip_distance_map* d_;
};

/* The window's immature points (dmvio_hip_immature_*) with the steps of FullSystem::activatePointsMT (FullSystem.cpp:604-773) that run on the device.  Does not own the
 * handle when constructed from one. */
class ImmaturePoints {
 public:
  ImmaturePoints(dmvio_hip_ctx* ctx, int capacity) : m_(dmvio_hip_immature_create(ctx, capacity)), own_(true) {}
  explicit ImmaturePoints(dmvio_hip_immature* handle) : m_(handle), own_(false) {}
  ~ImmaturePoints() { if (m_ && own_) dmvio_hip_immature_destroy(m_); }
  ImmaturePoints(const ImmaturePoints&) = delete;
  ImmaturePoints& operator=(const ImmaturePoints&) = delete;
  bool valid() const { return m_ != nullptr; }
  int size() const { return m_ ? dmvio_hip_immature_count(m_) : -1; }
  static float updateMinActDist(float currentMinActDist, int nPoints, float desiredPointDensity) {
    return dmvio_hip_min_act_dist_update(currentMinActDist, nPoints, desiredPointDensity);
  }
  /* the candidate loop (FullSystem.cpp:646-717): toOptimize.size(), or <0 */
  int selectForActivation(DistanceMap& map, const std::vector<float>& KRKi, const std::vector<float>& Kt, const std::vector<unsigned char>& flaggedForMarginalization,
                          int newestTag, float currentMinActDist, float minTraceQuality = 3.0f, int* nDeleted = nullptr) {
    int n = 0;
    if (!m_) return -1;
    const int r = dmvio_hip_immature_select_for_activation(m_, map.handle(), (int)(Kt.size() / 3), KRKi.data(), Kt.data(), flaggedForMarginalization.data(), newestTag,
                                                           currentMinActDist, minTraceQuality, &n, nDeleted);
    return r < 0 ? r : n;
  }
  /* decision per point (0 stays, 1 selected, 2 deleted) and the handle indices of toOptimize */
  bool activation(std::vector<int>& decision, std::vector<int>& order) {
    if (!m_) return false;
    const int n = dmvio_hip_immature_get_activation(m_, nullptr, nullptr);
    if (n < 0) return false;
    decision.assign((size_t)size(), 0); order.assign((size_t)n, 0);
    return dmvio_hip_immature_get_activation(m_, decision.data(), order.data()) >= 0;
  }
  /* optimizeImmaturePoint of the selection (FullSystem.cpp:723-756), results in toOptimize order: number of activated points, or <0 */
  int optimizeSelected(int F, const int* frameSlots, const double* worldToCam7, const double* aff2, const float* exposure, const double fxfycxcy[4], int minObs,
                       std::vector<int>& result, std::vector<float>& idepth, std::vector<int>& resState) {
    if (!m_) return -1;
    const int n = dmvio_hip_immature_get_activation(m_, nullptr, nullptr);
    if (n < 0) return n;
    result.assign((size_t)n, 0); idepth.assign((size_t)n, 0.f); resState.assign((size_t)n * F, -1);
    return dmvio_hip_immature_optimize_selected(m_, F, frameSlots, worldToCam7, aff2, exposure, fxfycxcy, minObs, result.data(), idepth.data(), resState.data());
  }
  /* the compaction (FullSystem.cpp:759-770): new number of points, or <0 */
  int removeMarked() { return m_ ? dmvio_hip_immature_remove_marked(m_) : -1; }
  /* a marginalised keyframe leaves: its points go, larger tags move down */
  int removeHost(int tag) { return m_ ? dmvio_hip_immature_remove_host(m_, tag) : -1; }
  bool types(std::vector<float>& myType) { myType.assign((size_t)std::max(size(), 0), 0.f); return m_ && dmvio_hip_immature_get_types(m_, myType.data()) == 0; }
  dmvio_hip_immature* handle() const { return m_; }

 private:
  dmvio_hip_immature* m_;
  bool own_;
};

/* FullSystem::activatePointsMT for several windows per call (dmvio_hip_activation_batch): W pairs of ImmaturePoints and DistanceMap of one context.  Every window ends in
 * the state its single calls leave; the results are read with the windows' own getters (ImmaturePoints::activation, DistanceMap::get).  A call is refused as a whole
 * (lastError()) before any window is touched. */
class ActivationBatch {
 public:
  ActivationBatch(dmvio_hip_ctx* ctx, int maxWindows) : b_(dmvio_hip_activation_batch_create(ctx, maxWindows)) {}
  ~ActivationBatch() { if (b_) dmvio_hip_activation_batch_destroy(b_); }
  ActivationBatch(const ActivationBatch&) = delete;
  ActivationBatch& operator=(const ActivationBatch&) = delete;
  bool valid() const { return b_ != nullptr; }
  /* makeDistanceMap (CoarseTracker.cpp:931-967) of every window: dm, n_hosts, the tables and the active points of each record */
  bool makeDistanceMaps(std::vector<dmvio_hip_activation_window>& windows) {
    return b_ && dmvio_hip_distance_map_make_batch(b_, (int)windows.size(), windows.data()) == 0;
  }
  /* the candidate loop (FullSystem.cpp:646-717) of every window; n_selected / n_deleted of each record are written */
  bool selectForActivation(std::vector<dmvio_hip_activation_window>& windows) {
    return b_ && dmvio_hip_immature_select_for_activation_batch(b_, (int)windows.size(), windows.data()) == 0;
  }
  /* optimizeImmaturePoint of every window's selection (FullSystem.cpp:723-756); the result arrays of each record are the caller's */
  bool optimizeSelected(std::vector<dmvio_hip_activation_optimize>& windows, const double fxfycxcy[4]) {
    return b_ && dmvio_hip_immature_optimize_selected_batch(b_, (int)windows.size(), windows.data(), fxfycxcy) == 0;
  }
  /* the compaction (FullSystem.cpp:759-770) of every handle: nLeft[i] = new number of points */
  bool removeMarked(const std::vector<ImmaturePoints*>& points, std::vector<int>& nLeft) {
    if (!b_) return false;
    std::vector<dmvio_hip_immature*> hs(points.size());
    for (size_t i = 0; i < points.size(); i++) { if (!points[i]) return false; hs[i] = points[i]->handle(); }
    nLeft.assign(points.size(), 0);
    return dmvio_hip_immature_remove_marked_batch(b_, (int)hs.size(), hs.data(), nLeft.data()) == 0;
  }

 private:
  dmvio_hip_activation_batch* b_;
};

/* FullSystem::traceNewCoarse for several windows per call (dmvio_hip_trace_batch): W ImmaturePoints of one context, each against its own new frame.  Every window ends in
 * the state its single call leaves; the points are read with the windows' own getters.  A call is refused as a whole (lastError()) before any window is touched. */
class TraceBatch {
 public:
  TraceBatch(dmvio_hip_ctx* ctx, int maxWindows) : b_(dmvio_hip_trace_batch_create(ctx, maxWindows)) {}
  ~TraceBatch() { if (b_) dmvio_hip_trace_batch_destroy(b_); }
  TraceBatch(const TraceBatch&) = delete;
  TraceBatch& operator=(const TraceBatch&) = delete;
  bool valid() const { return b_ != nullptr; }
  /* ImmaturePoint::traceOn (ImmaturePoint.cpp:76-437) of every window's points with the caller's tables; does not wait for the stream */
  bool trace(const std::vector<dmvio_hip_trace_tables_window>& windows) {
    return b_ && dmvio_hip_immature_trace_batch(b_, (int)windows.size(), windows.data()) == 0;
  }
  /* traceNewCoarse (FullSystem.cpp:541-584) of every window from its poses; wantCounts: counts6 of each record is written behind the call's one wait, otherwise the
   * call does not wait */
  bool traceNewCoarse(std::vector<dmvio_hip_trace_window>& windows, const double fxfycxcy[4], bool wantCounts = true) {
    return b_ && dmvio_hip_trace_new_coarse_batch(b_, (int)windows.size(), windows.data(), fxfycxcy, wantCounts ? 1 : 0) == 0;
  }

 private:
  dmvio_hip_trace_batch* b_;
};

/* CoarseTracker::trackNewestCoarse for the frames of several windows per call (dmvio_hip_track_multi): problem i is aligned against the reference its own tracker
 * holds, all of them in one launch.  The trackers are only read; every problem returns what CoarseTracker's own batch call returns for it at the same launch shape.  A call
 * is refused as a whole (lastError()) before anything is written. */
class TrackMulti {
 public:
  TrackMulti(dmvio_hip_ctx* ctx, int maxWindows, int maxProblems) : m_(dmvio_hip_track_multi_create(ctx, maxWindows, maxProblems)) {}
  ~TrackMulti() { if (m_) dmvio_hip_track_multi_destroy(m_); }
  TrackMulti(const TrackMulti&) = delete;
  TrackMulti& operator=(const TrackMulti&) = delete;
  bool valid() const { return m_ != nullptr; }
  struct Problem {
    int window;               /* index into the tracker list */
    int newSlot;
    float new_ab_exposure;
    SE3 lastToNew;            /* in / out */
    AffLight aff_g2l;         /* in / out */
    double minResForAbort[5]; /* NAN = no abort rule */
    double lastResiduals[5], lastFlowIndicators[3], H[64], b[8];
    bool good;
    int iterations;
  };
  bool track(const std::vector<const CoarseTracker*>& trackers, std::vector<Problem>& problems, int coarsestLvl) {
    if (!m_) return false;
    const size_t W = trackers.size(), B = problems.size();
    std::vector<dmvio_hip_tracker*> hs(W);
    for (size_t w = 0; w < W; w++) { if (!trackers[w]) return false; hs[w] = trackers[w]->handle(); }
    std::vector<int> win(B), slots(B), good(B), its(B);
    std::vector<float> ex(B);
    std::vector<double> pose(7 * B), aff(2 * B), mr(5 * B), lr(5 * B), fl(3 * B), H(64 * B), b(8 * B);
    for (size_t i = 0; i < B; i++) {
      const Problem& p = problems[i];
      win[i] = p.window; slots[i] = p.newSlot; ex[i] = p.new_ab_exposure;
      p.lastToNew.toPose7(&pose[7 * i]);
      aff[2 * i] = p.aff_g2l.a; aff[2 * i + 1] = p.aff_g2l.b;
      for (int k = 0; k < 5; k++) mr[5 * i + k] = p.minResForAbort[k];
    }
    if (dmvio_hip_tracker_track_multi(m_, (int)W, hs.data(), (int)B, win.data(), slots.data(), ex.data(), pose.data(), aff.data(), coarsestLvl, mr.data(), lr.data(), fl.data(),
                                      H.data(), b.data(), good.data(), its.data()) != 0)
      return false;
    for (size_t i = 0; i < B; i++) {
      Problem& p = problems[i];
      p.lastToNew.fromPose7(&pose[7 * i]);
      p.aff_g2l = AffLight(aff[2 * i], aff[2 * i + 1]);
      for (int k = 0; k < 5; k++) p.lastResiduals[k] = lr[5 * i + k];
      for (int k = 0; k < 3; k++) p.lastFlowIndicators[k] = fl[3 * i + k];
      for (int k = 0; k < 64; k++) p.H[k] = H[64 * i + k];
      for (int k = 0; k < 8; k++) p.b[k] = b[8 * i + k];
      p.good = good[i] != 0; p.iterations = its[i];
    }
    return true;
  }
  /* workgroups per problem: 0 = the library's choice */
  bool setLaunchShape(int lmCluster) { return m_ && dmvio_hip_track_multi_set_launch_shape(m_, lmCluster) == 0; }
  bool setResidualOnlyEvals(bool on) { return m_ && dmvio_hip_track_multi_set_residual_only_evals(m_, on ? 1 : 0) == 0; }
  bool lastLaunch(int& workgroupsPerProblem, int& threadsPerWorkgroup) const { return m_ && dmvio_hip_track_multi_last_launch(m_, &workgroupsPerProblem, &threadsPerWorkgroup) == 0; }
  bool lastWork(long long& evals, long long& pointEvals) const { return m_ && dmvio_hip_track_multi_last_work(m_, &evals, &pointEvals) == 0; }
  dmvio_hip_track_multi* handle() const { return m_; }

 private:
  dmvio_hip_track_multi* m_;
};

/* CoarseTracker::setCoarseTrackingRef + makeCoarseDepthL0 for several trackers of one context per call (dmvio_hip_set_ref_batch): every tracker ends as its own
 * single call would have left it; one upload, a number of launches that does not depend on the number of windows, one download, one wait.  A call is refused as a whole
 * (lastError()) before any tracker is touched. */
class SetRefBatch {
 public:
  SetRefBatch(dmvio_hip_ctx* ctx, int maxWindows, int maxPointsPerWindow) : b_(dmvio_hip_set_ref_batch_create(ctx, maxWindows, maxPointsPerWindow)) {}
  ~SetRefBatch() { if (b_) dmvio_hip_set_ref_batch_destroy(b_); }
  SetRefBatch(const SetRefBatch&) = delete;
  SetRefBatch& operator=(const SetRefBatch&) = delete;
  bool valid() const { return b_ != nullptr; }
  struct Window {
    const CoarseTracker* tracker;
    int refSlot;
    float ref_ab_exposure;
    AffLight ref_aff_g2l;
    std::vector<float> u, v, idepth, hdiF;   /* the window's points projected into the new reference, as dmvio_hip_tracker_set_ref takes them */
  };
  bool setCoarseTrackingRef(const std::vector<Window>& windows) {
    if (!b_) return false;
    std::vector<dmvio_hip_set_ref_window> win(windows.size());
    for (size_t i = 0; i < windows.size(); i++) {
      const Window& w = windows[i];
      if (!w.tracker || w.v.size() != w.u.size() || w.idepth.size() != w.u.size() || w.hdiF.size() != w.u.size()) return false;
      win[i].trk = w.tracker->handle(); win[i].ref_slot = w.refSlot; win[i].ref_exposure = w.ref_ab_exposure;
      win[i].ref_aff_a = w.ref_aff_g2l.a; win[i].ref_aff_b = w.ref_aff_g2l.b;
      win[i].n = (int)w.u.size(); win[i].u = w.u.data(); win[i].v = w.v.data(); win[i].idepth = w.idepth.data(); win[i].hdiF = w.hdiF.data();
    }
    return dmvio_hip_tracker_set_ref_batch(b_, (int)win.size(), win.data()) == 0;
  }
  struct BaWindow {
    const CoarseTracker* tracker;
    dmvio_hip_ba* ba;            /* the resident window the points are read from (dmvio_hip_tracker_set_ref_from_ba_batch) */
    int refSlot;
    float ref_ab_exposure;
    AffLight ref_aff_g2l;
    int nSelected;               /* out */
  };
  bool setCoarseTrackingRefFromBA(std::vector<BaWindow>& windows) {
    if (!b_) return false;
    std::vector<dmvio_hip_set_ref_ba_window> win(windows.size());
    for (size_t i = 0; i < windows.size(); i++) {
      const BaWindow& w = windows[i];
      if (!w.tracker) return false;
      win[i].trk = w.tracker->handle(); win[i].ba = w.ba; win[i].ref_slot = w.refSlot; win[i].ref_exposure = w.ref_ab_exposure;
      win[i].ref_aff_a = w.ref_aff_g2l.a; win[i].ref_aff_b = w.ref_aff_g2l.b; win[i].n_selected = 0;
    }
    if (dmvio_hip_tracker_set_ref_from_ba_batch(b_, (int)win.size(), win.data()) != 0) return false;
    for (size_t i = 0; i < windows.size(); i++) windows[i].nSelected = win[i].n_selected;
    return true;
  }
  bool lastWork(int& launches, int& uploads, int& downloads, int& waits) const { return b_ && dmvio_hip_set_ref_batch_last_work(b_, &launches, &uploads, &downloads, &waits) == 0; }
  dmvio_hip_set_ref_batch* handle() const { return b_; }

 private:
  dmvio_hip_set_ref_batch* b_;
};

}  // namespace dmvio_hip
#endif
