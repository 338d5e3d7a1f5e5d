// TEST INFRASTRUCTURE for tests/golden/make_pixel_select_golden.py — not product code, never part of build().
// extern "C" entry points into the reference's own PixelSelector (FullSystem/PixelSelector2.cpp) and FrameHessian::makeImages as compiled into oracle/_ref/libref.so.
// No arithmetic of the path lives here: it builds the reference's objects, calls their members and copies the results out.  Compiled by the generator with the flags
// and include paths of oracle/Makefile.ref, only where the reference's sources exist; the binary is never committed.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

// select / randomPattern / ths are private; the standard headers above are already in
#define private public
#define protected public
#include "util/NumType.h"
#include "util/settings.h"
#include "util/globalCalib.h"
#include "util/FrameShell.h"
#include "FullSystem/HessianBlocks.h"
#include "FullSystem/ImmaturePoint.h"
#include "FullSystem/PixelSelector2.h"
#undef private
#undef protected

using namespace dso;

namespace {
struct Glue {
	int w, h;
	CalibHessian HCalib;
	PixelSelector* sel = nullptr;
	FrameHessian* fh = nullptr;
	FrameShell* shell = nullptr;
	std::vector<float> map;
};
void dropFrame(Glue* g)
{
	if (!g->fh) return;
	g->fh->efFrame = 0;
	delete g->fh; delete g->shell;
	g->fh = nullptr; g->shell = nullptr;
}
}  // namespace

extern "C" {

void* psg_create(int w, int h, const float K4[4])
{
	Eigen::Matrix3f K = Eigen::Matrix3f::Identity();
	K(0, 0) = K4[0]; K(1, 1) = K4[1]; K(0, 2) = K4[2]; K(1, 2) = K4[3];
	std::streambuf* old = std::cout.rdbuf();
	std::ostringstream sink;
	std::cout.rdbuf(sink.rdbuf());
	setGlobalCalib(w, h, K);
	Glue* g = new Glue();
	g->w = w; g->h = h;
	g->sel = new PixelSelector(w, h);
	std::cout.rdbuf(old);
	g->map.assign((size_t)w * h, 0.f);
	return g;
}
void psg_destroy(void* p)
{
	Glue* g = (Glue*)p;
	dropFrame(g);
	delete g->sel;
	delete g;
}
int psg_levels(void*) { return pyrLevelsUsed; }
void psg_pattern(void* p, unsigned char* out) { Glue* g = (Glue*)p; memcpy(out, g->sel->randomPattern, (size_t)g->w * g->h); }
void psg_set_settings(float histCut, float histAdd, float downweight, int dirDist)
{
	setting_minGradHistCut = histCut; setting_minGradHistAdd = histAdd; setting_gradDownweightPerLevel = downweight; setting_selectDirectionDistribution = dirDist != 0;
}
int psg_get_potential(void* p) { return ((Glue*)p)->sel->currentPotential; }
void psg_set_potential(void* p, int pot) { ((Glue*)p)->sel->currentPotential = pot; }

// a new FrameHessian from the image (FrameHessian::makeImages); rows 0 and h-1 of the three absSquaredGrad planes the selector reads, which makeImages leaves
// unwritten, are zeroed
void psg_frame(void* p, const float* img, const float* B256)
{
	Glue* g = (Glue*)p;
	dropFrame(g);
	if (B256) memcpy(g->HCalib.B, B256, sizeof(float) * 256);
	else for (int i = 0; i < 256; i++) g->HCalib.B[i] = i;
	g->fh = new FrameHessian();
	g->shell = new FrameShell();
	g->shell->camToWorld = SE3();
	g->shell->aff_g2l = AffLight(0, 0);
	g->shell->marginalizedAt = g->shell->id = 0;
	g->shell->timestamp = 0;
	g->shell->incoming_id = 0;
	g->fh->shell = g->shell;
	g->fh->ab_exposure = 1.0f;
	std::vector<float> copy(img, img + (size_t)g->w * g->h);
	g->fh->makeImages(copy.data(), &g->HCalib);
	for (int l = 0; l < 3; l++)
	{
		memset(g->fh->absSquaredGrad[l], 0, sizeof(float) * wG[l]);
		memset(g->fh->absSquaredGrad[l] + (size_t)wG[l] * (hG[l] - 1), 0, sizeof(float) * wG[l]);
	}
	g->sel->gradHistFrame = 0;   // a new frame at a recycled address must not meet the cached histogram (:200)
}

// PixelSelector::makeMaps -> its return value; map as bytes, thsSmoothed / ths (nbW*nbH)
int psg_make_maps(void* p, float density, int recursionsLeft, float thFactor, unsigned char* map_out, float* ths, float* thsSmoothed)
{
	Glue* g = (Glue*)p;
	const int r = g->sel->makeMaps(g->fh, g->map.data(), density, recursionsLeft, false, thFactor);
	for (size_t i = 0; i < g->map.size(); i++) map_out[i] = (unsigned char)g->map[i];
	const int nb = (g->w / 16) * (g->h / 16);
	if (ths) memcpy(ths, g->sel->ths, sizeof(float) * nb);
	if (thsSmoothed) memcpy(thsSmoothed, g->sel->thsSmoothed, sizeof(float) * nb);
	return r;
}
// PixelSelector::select alone at a given potential (after a makeMaps / makeHists of the frame) -> (n2, n3, n4)
void psg_select(void* p, int pot, float thFactor, int counts3[3], unsigned char* map_out)
{
	Glue* g = (Glue*)p;
	if (g->sel->gradHistFrame != g->fh) g->sel->makeHists(g->fh);
	std::vector<float> m((size_t)g->w * g->h);
	Eigen::Vector3i n = g->sel->select(g->fh, m.data(), pot, thFactor);
	for (int k = 0; k < 3; k++) counts3[k] = n[k];
	if (map_out) for (size_t i = 0; i < m.size(); i++) map_out[i] = (unsigned char)m[i];
}
// wall time of FullSystem::makeNewTraces' work on this CPU (FullSystem.cpp:1640-1666): makeMaps (histogram included) + the ImmaturePoint constructors; the selector's
// potential is put back before every repetition.  -> median microseconds over `reps`; *n_points = points constructed
double psg_time_new_traces(void* p, float density, int reps, int* n_points)
{
	Glue* g = (Glue*)p;
	const int pot0 = g->sel->currentPotential;
	std::vector<double> us;
	int made = 0;
	for (int r = 0; r < reps; r++)
	{
		g->sel->currentPotential = pot0;
		g->sel->gradHistFrame = 0;
		const auto t0 = std::chrono::steady_clock::now();
		g->sel->makeMaps(g->fh, g->map.data(), density);
		std::vector<ImmaturePoint*> pts;
		for (int y = patternPadding + 1; y < hG[0] - patternPadding - 2; y++)
			for (int x = patternPadding + 1; x < wG[0] - patternPadding - 2; x++)
			{
				const int i = x + y * wG[0];
				if (g->map[i] == 0) continue;
				ImmaturePoint* impt = new ImmaturePoint(x, y, g->fh, g->map[i], &g->HCalib);
				if (!std::isfinite(impt->energyTH)) delete impt;
				else pts.push_back(impt);
			}
		const auto t1 = std::chrono::steady_clock::now();
		us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
		made = (int)pts.size();
		for (ImmaturePoint* q : pts) delete q;
	}
	g->sel->currentPotential = pot0;
	std::sort(us.begin(), us.end());
	if (n_points) *n_points = made;
	return us[us.size() / 2];
}

}  // extern "C"
