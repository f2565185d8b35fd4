// executor_trace_mod_main.cpp -- launch trace of the native step executor for the unpadded "*" stack (CoStGcnMod: ten blocks of
// stride 1 whose temporal convs wait k - 1 = 8 frames, csk_co_plan_set_delays), without a GPU.  The recording stubs, the fake
// buffers and the model builder are those of executor_trace_main.cpp, included as they are (its main() is renamed out of the
// way); tests/test_mod_cpu.py compares what this program prints with the Python engine's launches for the same model.
#define main executor_trace_scenarios_main
#include "executor_trace_main.cpp"
#undef main

int main() {
    const std::vector<Shape> MOD = {{3, 64, 1, NONE}, {64, 64, 1, IDENT}, {64, 64, 1, IDENT}, {64, 64, 1, IDENT}, {64, 128, 1, CONV},
                                    {128, 128, 1, IDENT}, {128, 128, 1, IDENT}, {128, 256, 1, CONV}, {256, 256, 1, IDENT}, {256, 256, 1, IDENT}};
    const int32_t delays[10] = {8, 8, 8, 8, 8, 8, 8, 8, 8, 8};
    const int mix[3] = {1, 3, 4};
    Options o;
    Model m = make(MOD, o);
    if (csk_co_plan_set_delays(m.plan, 10, delays)) { fprintf(stderr, "executor_trace_mod: %s\n", err_text); return 2; }
    printf("{");
    for (int done = 0, i = 0; done < 100; ++i) {
        const int r = mix[i % 3] < 100 - done ? mix[i % 3] : 100 - done;
        cycle(m, r);
        done += r;
    }
    emit("mod");
    // a refused delay leaves the plan as it was
    const int32_t bad[10] = {8, 8, 8, 9, 8, 8, 8, 8, 8, 8};
    calls.push_back("[\"set_delays\"," + I_(csk_co_plan_set_delays(m.plan, 10, bad)) + "," + I_(csk_co_plan_set_delays(m.plan, 9, delays)) + "]");
    emit("refused");
    csk_co_plan_destroy(m.plan);
    printf("}\n");
    return 0;
}
