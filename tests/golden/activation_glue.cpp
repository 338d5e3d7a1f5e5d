// TEST INFRASTRUCTURE for tests/golden/make_activation_golden.py — not product code, never part of build().
// extern "C" entry points into the reference's own CoarseDistanceMap (FullSystem/CoarseTracker.cpp) and FullSystem::activatePointsMT (FullSystem/FullSystem.cpp) as
// compiled into oracle/_ref/libref.so.  No arithmetic of the path lives here: it builds the reference's FrameHessian / PointHessian / ImmaturePoint objects from case
// data (through the window helpers of oracle/ref_glue.cpp, which libref.so exports), calls the reference's members and copies the results out.
// FullSystem::activatePointsMT_Reductor is defined HERE: libref.so is not linked -Bsymbolic and this library is loaded in front of it, so the reference's
// activatePointsMT calls this definition, which hands back the per-point optimisation results of the case instead of running optimizeImmaturePoint.
// Compiled by the generator with the flags and include paths of oracle/Makefile.ref, only where the reference's sources exist; the binary is never committed.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#define private public
#define protected public
#include "util/NumType.h"
#include "util/settings.h"
#include "util/globalCalib.h"
#include "util/FrameShell.h"
#include "OptimizationBackend/EnergyFunctional.h"
#include "OptimizationBackend/EnergyFunctionalStructs.h"
#include "FullSystem/FullSystem.h"
#include "FullSystem/HessianBlocks.h"
#include "FullSystem/ImmaturePoint.h"
#include "FullSystem/CoarseTracker.h"
#undef private
#undef protected

using namespace dso;

// oracle/ref_glue.cpp (in libref.so); the window object's first member is its FullSystem*
extern "C" {
void* ref_ba_create(int w, int h, const double fxfycxcy[4]);
void ref_ba_destroy(void* p);
int ref_ba_add_frame(void* p, const double pose7_w2c[7], double aff_a, double aff_b, float exposure, int frameID, const float* img);
int ref_ba_add_point(void* p, int host, float u, float v, float idepth, const float* color, const float* weights, int hasDepthPrior, float* color_out, float* weights_out);
}

namespace {
struct Glue {
	void* win = nullptr;
	FullSystem* fs = nullptr;
	std::map<const ImmaturePoint*, int> id;       // case id of every immature point
	std::map<const ImmaturePoint*, int> result;   // what the interposed reductor returns for it: 1 / 0 / -1
	std::vector<int> order;                        // ids of toOptimize, in order
};
Glue* g_cur = nullptr;
}  // namespace

// the interposed member (FullSystem.cpp:589-600): results come from the case; an activated point is the reference's own PointHessian constructor
void FullSystem::activatePointsMT_Reductor(std::vector<PointHessian*>* optimized, std::vector<ImmaturePoint*>* toOptimize, int min, int max, Vec10* stats, int tid)
{
	Glue* g = g_cur;
	for (int k = min; k < max; k++)
	{
		ImmaturePoint* ip = (*toOptimize)[k];
		g->order.push_back(g->id.at(ip));
		const int r = g->result.at(ip);
		if (r == 1)
		{
			PointHessian* ph = new PointHessian(ip, &Hcalib);
			ph->setPointStatus(PointHessian::ACTIVE);
			(*optimized)[k] = ph;
		}
		else (*optimized)[k] = r == 0 ? (PointHessian*)0 : (PointHessian*)((long)(-1));
	}
}

extern "C" {

void* ag_create(int w, int h, const double K4[4])
{
	Glue* g = new Glue();
	g->win = ref_ba_create(w, h, K4);
	g->fs = *(FullSystem**)g->win;
	return g;
}
void ag_destroy(void* p)
{
	Glue* g = (Glue*)p;
	ref_ba_destroy(g->win);
	delete g;
}
int ag_add_frame(void* p, const double w2c7[7], const float* img, int flagged)
{
	Glue* g = (Glue*)p;
	const int idx = ref_ba_add_frame(g->win, w2c7, 0.0, 0.0, 1.0f, (int)g->fs->frameHessians.size(), img);
	g->fs->frameHessians[idx]->flaggedForMarginalization = flagged != 0;
	return idx;
}
void ag_add_active(void* p, int host, int n, const float* u, const float* v, const float* idepth)
{
	Glue* g = (Glue*)p;
	for (int i = 0; i < n; i++) ref_ba_add_point(g->win, host, u[i], v[i], idepth[i], 0, 0, 0, 0, 0);
}
// ImmaturePoint constructor at integer pixels of keyframe `host`, then the state a sequence of traces would have left, from the case
void ag_add_immature(void* p, int host, int n, const int* id, const int* u, const int* v, const float* my_type, const float* idepth_min, const float* idepth_max,
                     const float* quality, const float* interval, const int* status, const int* result)
{
	Glue* g = (Glue*)p;
	FrameHessian* fh = g->fs->frameHessians[host];
	for (int i = 0; i < n; i++)
	{
		ImmaturePoint* ip = new ImmaturePoint(u[i], v[i], fh, my_type[i], &g->fs->Hcalib);
		ip->idepth_min = idepth_min[i]; ip->idepth_max = idepth_max[i]; ip->quality = quality[i]; ip->lastTracePixelInterval = interval[i];
		ip->lastTraceStatus = (ImmaturePointStatus)status[i];
		fh->immaturePoints.push_back(ip);
		g->id[ip] = id[i]; g->result[ip] = result[i];
	}
}
void ag_get_map(void* p, float* out)
{
	Glue* g = (Glue*)p;
	memcpy(out, g->fs->coarseDistanceMap->fwdWarpedIDDistFinal, sizeof(float) * (size_t)(wG[1] * hG[1]));
}
// CoarseDistanceMap::makeK + makeDistanceMap against the newest keyframe (FullSystem.cpp:638-639)
void ag_make_map(void* p, float* out)
{
	Glue* g = (Glue*)p;
	g->fs->coarseDistanceMap->makeK(&g->fs->Hcalib);
	g->fs->coarseDistanceMap->makeDistanceMap(g->fs->frameHessians, g->fs->frameHessians.back());
	if (out) ag_get_map(p, out);
}
void ag_add_into(void* p, int u, int v) { ((Glue*)p)->fs->coarseDistanceMap->addIntoDistFinal(u, v); }
// what makeK left: K[1] and Ki[0], row-major
void ag_level_k(void* p, float* K1, float* Ki0)
{
	CoarseDistanceMap* d = ((Glue*)p)->fs->coarseDistanceMap;
	for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { K1[3 * r + c] = d->K[1](r, c); Ki0[3 * r + c] = d->Ki[0](r, c); }
}
// the reference's FullSystem::activatePointsMT.  nPoints >= 0 replaces ef->nPoints for the controller during the call.  -> toOptimize.size(); order_out = case ids;
// *cur_after = currentMinActDist after the call; *usec = wall time of the call
int ag_activate(void* p, float minActDist_before, int nPoints, float desiredDensity, float minTraceQuality, float* cur_after, int* order_out, double* usec)
{
	Glue* g = (Glue*)p;
	FullSystem* fs = g->fs;
	setting_desiredPointDensity = desiredDensity;
	setting_minTraceQuality = minTraceQuality;
	fs->currentMinActDist = minActDist_before;
	const int realPoints = fs->ef->nPoints;
	if (nPoints >= 0) fs->ef->nPoints = nPoints;
	g->order.clear();
	g_cur = g;
	const auto t0 = std::chrono::steady_clock::now();
	fs->activatePointsMT();
	const auto t1 = std::chrono::steady_clock::now();
	g_cur = nullptr;
	if (nPoints >= 0) fs->ef->nPoints += realPoints - nPoints;
	if (cur_after) *cur_after = fs->currentMinActDist;
	if (usec) *usec = std::chrono::duration<double, std::micro>(t1 - t0).count();
	if (order_out) for (size_t k = 0; k < g->order.size(); k++) order_out[k] = g->order[k];
	setting_desiredPointDensity = 2000; setting_minTraceQuality = 3;
	return (int)g->order.size();
}
// a host's immaturePoints after the call: case ids in list order
int ag_list(void* p, int host, int* ids)
{
	Glue* g = (Glue*)p;
	FrameHessian* fh = g->fs->frameHessians[host];
	for (size_t i = 0; i < fh->immaturePoints.size(); i++) ids[i] = g->id.at(fh->immaturePoints[i]);
	return (int)fh->immaturePoints.size();
}
int ag_num_active(void* p, int host) { return (int)((Glue*)p)->fs->frameHessians[host]->pointHessians.size(); }
int ag_ef_points(void* p) { return ((Glue*)p)->fs->ef->nPoints; }

}  // extern "C"
