// The reference's ViewMode::Textures (src/main.cpp:752-761) written against the facade: loadMesh of a textured
// OBJ -> BoundingVolumeHierarchy(&scene) -> renderRayTracing(scene, camera, bvh, screen, /*textureDebugging=*/true),
// and the same view for a batch of cameras (renderTextureViews).  Writes the frame as raw float32 to
// <out>/texture_frame.bin for tests/test_texture_view.py to compare with the Python call's.
// Exit code 0 = ok, 3 = no GPU (the constructor threw, as it must without a device).
#include <cstdio>
#include <string>
#include <vector>

#include "rt_facade.hpp"

using namespace rt::facade;

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string sceneDir = argv[1], out = argv[2];
    const int W = 48, H = 32;
    Window window{W, H};
    Scene scene;
    scene.meshes = loadMesh(sceneDir + "/checker.obj");
    scene.spheres.push_back(Sphere{vec3(0.0f, 0.45f, -0.5f), 0.4f, Material{vec3(0.1f), vec3(0.8f), 0.0f, 1.0f, {}}});
    scene.pointLights.push_back(PointLight{vec3(0.0f, 2.0f, 1.0f), vec3(1.0f)});
    size_t textured = 0;
    for (const Mesh& m : scene.meshes) textured += m.material.kdTexture.has_value() ? 1 : 0;
    std::printf("meshes=%zu textured=%zu spheres=%zu\n", scene.meshes.size(), textured, scene.spheres.size());
    if (textured == 0) return 4;
    try {
        BoundingVolumeHierarchy bvh{&scene};
        Trackball camera{&window, radians(50.0f), 3.0f};
        camera.setCamera(vec3(0.0f, 0.0f, 0.0f), radians(vec3(20.0f, 20.0f, 0.0f)), 3.0f);
        // the view's knobs; useTextures stays off: the view samples regardless (src/main.cpp:95-105)
        textureFiltering = TextureFiltering::Trilinear;
        outOfBoundsRuleX = OutOfBoundsRule::Repeat;
        outOfBoundsRuleY = OutOfBoundsRule::Clamp;
        textureBorderColor = vec3(0.2f, 0.3f, 0.4f);

        Screen screen{W, H};
        renderRayTracing(scene, camera, bvh, screen, /*textureDebugging=*/true);
        FILE* f = std::fopen((out + "/texture_frame.bin").c_str(), "wb");
        if (!f) return 5;
        std::fwrite(screen.textureData().data(), sizeof(float), screen.textureData().size(), f);
        std::fclose(f);

        // a batch: every view equals its own renderRayTracing(..., true) call, bit for bit
        std::vector<Trackball> cams(3, camera);
        cams[1].setCamera(vec3(0.0f), vec3(0.34906584f, 0.84906584f, 0.0f), 3.0f);
        cams[2].setCamera(vec3(0.0f), vec3(0.6f, -0.4f, 0.0f), 3.0f);
        std::vector<std::vector<float>> views;
        renderTextureViews(scene, cams, bvh, W, H, views);
        int same = 0;
        for (size_t v = 0; v < cams.size(); ++v) {
            Screen one{W, H};
            renderRayTracing(scene, cams[v], bvh, one, true);
            same += (one.textureData() == views[v]) ? 1 : 0;
        }
        std::printf("views_identical=%d/%d\n", same, (int)cams.size());
        std::printf("done\n");
        return 0;
    } catch (const std::exception& e) {
        std::printf("no device: %s\n", e.what());
        return 3;
    }
}
